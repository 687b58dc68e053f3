"""CPU suite: the sizes and the rows of tests/piece_cases.py are what tests/test_gpu_batch_pieces.py's assertions rest on -- checked
with the models alone, before any of them reaches a device.  These are conditions on the inputs, not measurements of the library."""
import math

import numpy as np
import pytest

import piece_cases as pc


def test_the_three_splits():
    """piece_rows restated: the default cut, the many-piece cut and the one-piece calls, for every call's row width"""
    for family in pc.FAMILIES:
        arrays = pc.family_rows(family)
        for c in pc.CALLS[family]:
            row = pc.staged_row(c, arrays)
            assert pc.split(pc.DEFAULT_N, row) == [65536, 65536, 3], c.label
            assert pc.split(pc.CUT_N, row, pc.CUT_KNOBS) == [5632] * 23 + [1537], c.label
            assert pc.split(pc.SMALL_N, row, pc.CUT_KNOBS) == [pc.SMALL_N], c.label
            assert pc.split(pc.PIECE_THRESHOLD - 1, row) == [pc.PIECE_THRESHOLD - 1], "below 2^17 rows nothing is cut"
    assert sum(pc.split(pc.CUT_N, 64, pc.CUT_KNOBS)) == pc.CUT_N and len(pc.split(pc.CUT_N, 64, pc.CUT_KNOBS)) == pc.MOST_PIECES > 8
    assert set(pc.PIECE_SIZES) == {5632, 65536}
    assert pc.knob_values({}) == (8, 1 << 16) and pc.knob_values(pc.CUT_KNOBS) == (24, 256)
    assert pc.knob_values({"C25519_AMD_BATCH_PIECES": "1", "C25519_AMD_PIECE_MIN_ROWS": "255"}) == (8, 1 << 16), "out of range: the default"


def test_the_cap_cut():
    """ed25519_HashToScalar_batch stages msg_size + 32 bytes a row: 4096 rows fill a buffer set, five more make a second piece"""
    row = pc.CAP_MSG_SIZE + 32
    assert pc.cap_rows(row) == 4096
    assert pc.CAP_MSG_SIZE % 16 and 4096 * row > pc.STAGING_CAP
    assert pc.CAP_N < pc.PIECE_THRESHOLD and pc.split(pc.CAP_N, row) == [4096, pc.CAP_N - 4096] and 1 <= pc.CAP_N - 4096 <= 8
    assert all(pc.cap_rows(m + 32) > 4096 for m in range(pc.CAP_MSG_SIZE - 64, pc.CAP_MSG_SIZE) if m % 16), "the smallest such call"
    rows = pc.cap_rows_set()
    assert rows["cap_msg"].shape == (pc.CAP_PERIOD, pc.CAP_MSG_SIZE) and pc.period_ok(pc.CAP_PERIOD)
    assert len({r.tobytes() for r in rows["cap"]}) == pc.CAP_PERIOD
    assert pc.staged_row(pc.CAP_CALL, rows) == row


def test_the_period_condition():
    assert [p for p in range(20, 40) if pc.period_ok(p)] == [25, 27, 29, 31, 35, 37, 39]
    assert pc.usable_period(1034) == 1033 and pc.usable_period(250) == 249 and pc.usable_period(4183) == 4183
    for p in (29, 53, 249, 4183):
        assert 0 not in pc.shifts(p)


def _calls_of(family):
    return pc.CALLS[family] + pc.SMALL_AFTER.get(family, [])


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_every_set_meets_the_period_condition(family):
    """period > 24 and coprime to both piece sizes, all arrays of a call of one length -- and, stronger, for every distance a
    misplaced piece can be off by, some row of every output differs from the row that far away"""
    arrays = pc.family_rows(family)
    for c in _calls_of(family):
        period = pc.period_of(c, arrays)
        assert pc.period_ok(period), (c.label, period)
        assert period > pc.MOST_PIECES and math.gcd(period, 5632 * 65536) == 1
        for key in pc.keys_of(c, "out"):
            want = arrays[key]
            for s in pc.shifts(period):
                assert (want != np.roll(want, -s, axis=0)).any(), (c.label, key, s)
        distinct = len({tuple(arrays[k][i].tobytes() for k in pc.keys_of(c, "in")) for i in range(period)})
        assert distinct > pc.MOST_PIECES, (c.label, "calls that share a set may see a value twice, but never fewer values than pieces")


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_ok_and_flags_take_both_values(family):
    arrays = pc.family_rows(family)
    seen = 0
    for c in _calls_of(family):
        for key in pc.keys_of(c, "out"):
            want = arrays[key]
            if want.ndim == 1:
                seen += 1
                assert want.dtype in (np.int32, np.uint32) and len(np.unique(want)) >= 2, (c.label, key)
                if want.dtype == np.int32:
                    assert set(np.unique(want)) == {0, 1}, (c.label, key)
    assert seen == {"keys": 4, "group": 5, "ristretto255": 4, "scalar": 2, "h2c": 0, "vrf": 3, "sign_indexed": 0}[family]


def test_the_rows_hold_what_makes_ok_vary():
    import key_model
    import vrf_model
    from scalar_model import L, from_rows
    keys = pc.family_rows("keys")
    assert {3, 11} <= set(int(f) for f in keys["flags"]) and any(not f & key_model.DECODES for f in keys["flags"]), "mixed-order, honest, undecodable"
    assert any(f & key_model.SMALL_ORDER for f in keys["flags"])
    sc = pc.family_rows("scalar")
    zero = [v % L == 0 for v in from_rows(sc["x"])]
    assert any(v and zero[i] for i, v in enumerate(from_rows(sc["x"]))), "s = 0 mod L with s != 0"
    assert np.array_equal(sc["ok"] == 0, np.array(zero))
    vrf = pc.family_rows("vrf")
    assert len(vrf["ok_r"]) == len(vrf_model.rejections()["labels"]) == 29 and 2 <= int(vrf["ok_r"].sum()) < 29
    assert 0 < int(vrf["ok_v"].sum()) < pc.VRF_PERIOD and not vrf["ok_v"][1::3].any() and vrf["ok_v"][0::3].all()
    assert not vrf["beta_v"][vrf["ok_v"] == 0].any()
    rist = pc.family_rows("ristretto255")
    assert 0 < int(rist["valid"].sum()) < len(rist["valid"]) and 0 < int(rist["q_ok"].sum()) < len(rist["q_ok"])
    grp = pc.family_rows("group")
    assert 0 < int(grp["q_ok"].sum()) < len(grp["q_ok"]) and 0 < int(grp["sum_ok"].sum()) < len(grp["sum_ok"])


def test_message_lengths_sit_at_the_block_edges():
    import h2c_model
    import vrf_model
    residues = {k: (m + d + 4) % 128 for k, (d, m) in pc.H2C_SHAPES.items()}
    assert {residues[k] for k in ("h2curve", "e2curve", "h2group", "h2scalar")} == {127, 0, 112, 1}
    assert all(d in h2c_model.DST_LENGTHS for d, _ in pc.H2C_SHAPES.values())
    assert sum(1 for _, m in pc.H2C_SHAPES.values() if m % 4) >= 3, "rows that start unaligned inside the staging buffer"
    assert [(32 + a + len(vrf_model.DST) + 4) % 128 for a in pc.VRF_ALPHAS] == [127, 0]
    assert pc.VRF_ALPHAS[0] % 4 and vrf_model.REJECT_ALPHA % 4 and pc.SIGN_MSG_SIZE % 4 and pc.SIGN_MSG_SIZE == 47
    h2c = pc.family_rows("h2c")
    assert h2c["xmd"].shape == (pc.H2C_FAST_PERIOD, 129)
    for key, (dst_len, msg_size) in pc.H2C_SHAPES.items():
        assert h2c[key + "_msg"].shape[1] == msg_size and h2c[key + "_dst"].shape == (dst_len,)


def test_the_table_names_every_call_the_issue_lists():
    from curve25519_amd import _lib
    symbols = {c.symbol for f in pc.FAMILIES for c in pc.CALLS[f]}
    assert len(symbols) == 3 + 6 + 6 + 9 + 6 + 3 + 1
    assert symbols <= set(_lib.SIGNATURES), symbols - set(_lib.SIGNATURES)
    for f in pc.FAMILIES:
        for c in _calls_of(f) + [pc.CAP_CALL]:
            assert len(c.args) == len(_lib.SIGNATURES[c.symbol]), c.label
    variants = pc.in_place_variants("scalar")
    assert sorted((c.symbol[len("ed25519_Scalar"):-len("_batch")], i) for c, _, i in variants) == sorted(
        [("Negate", "x"), ("Complement", "x"), ("Invert", "x")] + [(k, i) for k in ("Add", "Sub", "Mul") for i in "xy"]
        + [("MulAdd", i) for i in "xyz"])
    assert all(not pc.in_place_variants(f) for f in pc.FAMILIES if f != "scalar")


def test_the_runner_reports_what_goes_wrong():
    """run_call against a stand-in library: a clean call, rows put one piece too far, a written guard row, a changed input"""
    import ctypes as C
    arrays = dict(x=np.arange(29 * 32, dtype=np.uint8).reshape(29, 32), neg=(255 - np.arange(29 * 32, dtype=np.uint8)).reshape(29, 32))
    c = pc.call("negate", pc.O("neg"), pc.I("x"), pc.N)
    n, chunk = 1000, 300

    def view(p, rows):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(rows, 32))

    class Lib:
        mode = "clean"

        def negate(self, out, src, count):
            o, s = view(out, count + 1), view(src, count)
            o[:count] = 255 - s
            if self.mode == "shifted":
                o[chunk:count] = 255 - s[np.arange(chunk, count) - 1]
            if self.mode == "guard":
                o[count, 0] = 0
            if self.mode == "input":
                s[7, 0] ^= 1
            return 0

        def c25519_amd_last_error(self):
            return b""

    lib = Lib()
    assert pc.run_call(lib, c, arrays, n, env={}) == dict(call="negate", n=n, chunk=n, rc=0, differ=0, first=[], guard=True,
                                                          inputs_unchanged=True, error="")
    lib.mode = "shifted"
    r = pc.run_call(lib, c, arrays, n, env={})
    assert r["differ"] == n - chunk and r["first"][0] == ["neg", chunk, 0] and pc.failures([r]) == [r]
    for mode, field in (("guard", "guard"), ("input", "inputs_unchanged")):
        lib.mode = mode
        r = pc.run_call(lib, c, arrays, n, env={})
        assert r[field] is False and pc.failures([r]) == [r]
    lib.mode = "clean"
    r = pc.run_call(lib, c, arrays, n, env={}, alias=("neg", "x"))
    assert not pc.failures([r]) and r["call"] == "negate, neg over x"
