"""GPU suite (MI355X): the strict verification calls -- ed25519_VerifySignature_strict_* and ed25519_Verify_Check_strict_*.  Expected
verdicts: the strict rule in Python big integers (tests/strict_cases.py) on top of the reference's verdict (the oracle's) or, where
the plain call is the reference's stand-in (ragged messages, Verify_Check contexts), on top of the plain call's verdict.  Every
dispatch shape is covered: per wave (n <= 1024), quads (1025 .. 32768), one lane per element, and the slow list under a low lattice
cap; keys off the curve must never reach the reference-order kernel."""
import threading

import numpy as np
import pytest

import strict_cases as sc
from curve25519_amd import _lib
from vectors import L

pytestmark = pytest.mark.gpu

SIZES = (1, 1024, 1025, 4096, 32768, 32769, 65537)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def honest(api, n, seed, mlen=32):
    rng = np.random.default_rng(seed)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    return api.ed25519_SignMessage(priv, msg), pub, msg


@pytest.fixture(scope="module")
def mixed(api, oracle):
    """65537 elements: honest signatures with the edge set spread over them (every 97th row from 1 on) and corrupted ones; row 0
    honest.  (sig, pk, msg, strict verdicts)"""
    n = SIZES[-1]
    sig, pk, msg = honest(api, n, 0x57A1)
    esig, epk, emsg = sc.edge_cases(oracle)
    pos = np.arange(1, n, 97)[:len(esig)]
    sig[pos], pk[pos], msg[pos] = esig[:len(pos)], epk[:len(pos)], emsg[:len(pos)]
    sig[5::101, 7] ^= 0x10
    ref = oracle.ed25519_verify(sig, pk, msg, threads=16)
    return sig, pk, msg, sc.strict_rule(sig, pk, ref)


@pytest.mark.parametrize("knob", [None, ("QUAD_MAX", 0), ("COOP_MAX", 0), ("VERIFY_LAT_CAP_BITS", 100)])
def test_strict_verdicts_equal_the_model(api, mixed, knob):
    sig, pk, msg, want = mixed
    assert want[0] == 1 and want.sum() > SIZES[-1] // 2 and (want == 0).sum() > 700
    for n in SIZES:
        if knob:
            with _lib.tunable(*knob):
                got = api.ed25519_VerifySignature_strict(sig[:n], pk[:n], msg[:n])
        else:
            got = api.ed25519_VerifySignature_strict(sig[:n], pk[:n], msg[:n])
        assert np.array_equal(got, want[:n]), (knob, n, np.nonzero(got != want[:n])[0][:10])
    if knob == ("VERIFY_LAT_CAP_BITS", 100):
        with _lib.tunable(*knob):
            api.ed25519_VerifySignature_strict(sig, pk, msg)
            assert _lib.load().c25519_amd_verify_last_slow_elements() > 1000      # over-long vectors did take the slow list


PATHS = {"wave": (), "quad": (("COOP_MAX", 0), ("QUAD_MIN", 0)), "lane": (("COOP_MAX", 0), ("QUAD_MAX", 0)),
         "slow": (("COOP_MAX", 0), ("QUAD_MAX", 0), ("VERIFY_LAT_CAP_BITS", 100))}


def strict_on(api, path, *args):
    import contextlib
    with contextlib.ExitStack() as st:
        for k, v in PATHS[path]:
            st.enter_context(_lib.tunable(k, v))
        return api.ed25519_VerifySignature_strict(*args)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_edge_set_alone_on_every_path(api, oracle, path):
    sig, pk, msg = sc.edge_cases(oracle, seed=6)
    want = sc.strict_rule(sig, pk, oracle.ed25519_verify(sig, pk, msg))
    got = strict_on(api, path, sig, pk, msg)
    assert np.array_equal(got, want), (path, np.nonzero(got != want)[0][:10])
    assert want.sum() >= 16


def test_honest_inputs_equal_the_plain_device_call(api):
    import torch
    for n in (1, 1024, 4096, 65536):
        sig, pk, msg = honest(api, n, 0x57A2 + n)
        sig[3::17, 50] ^= 1
        t = [torch.from_numpy(a).cuda() for a in (sig, pk, msg)]
        plain = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        strict = torch.full((n, 1), 7, dtype=torch.int32, device="cuda")
        api.ed25519_VerifySignature_dev(plain, *t)
        api.ed25519_VerifySignature_strict_dev(strict, *t)
        assert torch.equal(plain, strict), n
        assert int(plain.sum()) == n - len(range(3, n, 17))


@pytest.mark.parametrize("n", [1000, 4096, 65536])
def test_off_curve_keys_never_reach_the_slow_list(api, n):
    sig, pk, msg = honest(api, n, 0x57A3)
    hsig, hpk = sc.hostile(sig, pk, "offcurve")
    got = api.ed25519_VerifySignature_strict(hsig, hpk, msg)
    assert _lib.load().c25519_amd_verify_last_slow_elements() == 0
    assert not got[1::2].any() and got[0::2].all()
    api.ed25519_VerifySignature(hsig, hpk, msg)
    assert _lib.load().c25519_amd_verify_last_slow_elements() == len(range(1, n, 2))      # the plain call lists them


@pytest.mark.parametrize("kind", ["s_plus_l", "small_key"])
def test_hostile_mixes_are_rejected(api, kind):
    sig, pk, msg = honest(api, 65536, 0x57A4)
    hsig, hpk = sc.hostile(sig, pk, kind)
    assert not api.ed25519_VerifySignature_strict(hsig, hpk, msg).any()
    assert _lib.load().c25519_amd_verify_last_slow_elements() == 0
    if kind == "s_plus_l":
        assert api.ed25519_VerifySignature(hsig, hpk, msg).all()                # the reference accepts S + L


def test_ragged_forms(api):
    import torch
    rng = np.random.default_rng(0x57A5)
    for n in (700, 5000, 40000):
        pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        lens = rng.integers(0, 300, n)
        msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
        sig = api.ed25519_SignMessage_ragged(priv, msgs)
        hsig, _ = sc.hostile(sig[0::3], pub[0::3], "s_plus_l")
        sig[0::3] = hsig
        _, hpk = sc.hostile(sig[1::5], pub[1::5], "small_key")
        pub[1::5] = hpk
        _, hpk = sc.hostile(sig[2::14], pub[2::14], "offcurve")
        pub[2::14] = hpk
        plain = api.ed25519_VerifySignature_ragged(sig, pub, msgs)
        want = sc.strict_rule(sig, pub, plain)
        assert want.sum() > n // 3
        assert np.array_equal(api.ed25519_VerifySignature_strict_ragged(sig, pub, msgs), want), n
        flat = np.frombuffer(b"".join(msgs), np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        d = [torch.from_numpy(a.copy()).cuda() for a in (sig, pub, flat, offs)]
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.load().ed25519_VerifySignature_strict_ragged_dev(out.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                                  d[3].data_ptr(), n, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), n


def test_batch_in_pieces_and_two_threads(api, mixed):
    sig, pk, msg, want = mixed
    reps = 4                                                         # 262148 rows: the host pipeline cuts them into pieces
    big = [np.concatenate([a] * reps) for a in (sig, pk, msg)]
    assert np.array_equal(api.ed25519_VerifySignature_strict(*big), np.concatenate([want] * reps))
    out, errs = {}, []

    def work(k):
        try:
            lo = 9000 * k
            for _ in range(3):
                out[k] = api.ed25519_VerifySignature_strict(sig[lo:lo + 30000], pk[lo:lo + 30000], msg[lo:lo + 30000])
        except Exception as e:                                        # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for k in range(2):
        assert np.array_equal(out[k], want[9000 * k:9000 * k + 30000]), k


# ---- ed25519_Verify_Check_strict_* ------------------------------------------------------------------------------------------------

def _context_cases(api, oracle):
    """{name: (ctx bytes, [(sig, msg)] honest under the key where one can be made)} for an honest key, a mixed-order key, a key of
    small order, a non-canonical encoding (y >= p), a key off the curve, and a tampered honest context"""
    import random
    rnd = random.Random(0x57A6)
    rng = np.random.default_rng(0x57A6)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (1, 32), dtype=np.uint8))
    a = rnd.getrandbits(252) % L
    T8 = sc.ed_order8_point()
    mixed_pk = sc.ed_enc(sc.ed_add(sc.ed_mul(a, sc.ED_B), sc.ed_mul(3, T8)))
    small = sc.small_order_encodings()[5][0]
    off = next(y for y in range(2, 64) if sc.ed_decode(y, 0) is None).to_bytes(32, "little")
    noncanon = (sc.P + next(y for y in range(2, 19) if sc.ed_decode(y, 0) is not None)).to_bytes(32, "little")   # y + p: on the curve
    keys = {"honest": pub[0].tobytes(), "mixed": mixed_pk, "small": small, "noncanon": noncanon, "offcurve": off}
    ctxs = {k: api.ed25519_Verify_Init(np.frombuffer(v, np.uint8)[None, :])[0] for k, v in keys.items()}
    t = ctxs["honest"].copy()
    t[32 + 128 * 3 + 5] ^= 1
    ctxs["tampered"] = t
    return ctxs, priv[0], a, mixed_pk


def _pairs(api, oracle, n, priv, a, mixed_pk, key, seed):
    """n (sig, msg): honest under `key`'s signer (the device-made key; the mixed-order key by big-integer signing for the first few),
    S + L in every 5th, a small-order R in every 7th, a corrupted byte in every 11th"""
    import random
    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig = api.ed25519_SignMessage(np.stack([priv] * n), msg)
    if key == "mixed":
        for i in range(min(n, 24)):
            Rb, S = sc._sign_with(a, 3, mixed_pk, msg[i].tobytes(), rnd)
            sig[i] = np.frombuffer(Rb + S.to_bytes(32, "little"), np.uint8)
    for i in range(0, n, 5):
        S = int.from_bytes(sig[i, 32:].tobytes(), "little") + L
        sig[i, 32:] = np.frombuffer(S.to_bytes(32, "little"), np.uint8)
    encs = [e for e, _ in sc.small_order_encodings()]
    for j, i in enumerate(range(3, n, 7)):
        sig[i, :32] = np.frombuffer(encs[j % len(encs)], np.uint8)
    sig[6::11, 40] ^= 2
    return sig, msg


@pytest.mark.parametrize("n", [1, 1024, 4096, 65536])
def test_verify_check_strict_on_every_context(api, oracle, n):
    ctxs, priv, a, mixed_pk = _context_cases(api, oracle)
    for name, ctx in ctxs.items():
        sig, msg = _pairs(api, oracle, n, priv, a, mixed_pk, name, 0x57A7 + n)
        plain = api.ed25519_Verify_Check(ctx, sig, msg)
        want = sc.strict_rule(sig, np.stack([ctx[:32]] * n), plain)
        got = api.ed25519_Verify_Check_strict(ctx, sig, msg)
        assert np.array_equal(got, want), (name, n, np.nonzero(got != want)[0][:10])
        if name in ("honest", "tampered") and n > 1:
            assert plain[0::5].any() and not got[0::5].any()                   # S + L: the reference accepts, strict does not
        if name == "honest" and n > 7:
            assert want.sum() > n // 2
        if name == "mixed" and n > 1:
            assert want[:24].sum() >= 10                                       # mixed-order keys keep their right signatures
        if name == "honest" and n == 65536:
            assert _lib.load().c25519_amd_verify_check_last_wide() == 1       # the key's wide comb was built
    if n == 65536:                                                             # the honest context's comb, built by a call of 2^16 ...
        sig, msg = _pairs(api, oracle, n, priv, a, mixed_pk, "honest", 0x57AA)
        api.ed25519_Verify_Check_strict(ctxs["honest"], sig, msg)
    sig, msg = _pairs(api, oracle, 4096, priv, a, mixed_pk, "honest", 0x57A8)
    want = sc.strict_rule(sig, np.stack([ctxs["honest"][:32]] * 4096), api.ed25519_Verify_Check(ctxs["honest"], sig, msg))
    assert np.array_equal(api.ed25519_Verify_Check_strict(ctxs["honest"], sig, msg), want)
    if n == 65536:
        assert _lib.load().c25519_amd_verify_check_last_wide() == 1           # ... and remembered by the next, smaller call


def test_verify_check_strict_device_form(api, oracle):
    import torch
    ctxs, priv, a, mixed_pk = _context_cases(api, oracle)
    for name in ("honest", "small", "offcurve"):
        for n in (1, 2000):
            sig, msg = _pairs(api, oracle, n, priv, a, mixed_pk, name, 0x57A9)
            want = api.ed25519_Verify_Check_strict(ctxs[name], sig, msg)
            out = torch.full((n, 1), 7, dtype=torch.int32, device="cuda")
            api.ed25519_Verify_Check_strict_dev(out, torch.from_numpy(ctxs[name][None, :].copy()).cuda(), torch.from_numpy(sig).cuda(),
                                                torch.from_numpy(msg).cuda())
            assert np.array_equal(out.cpu().numpy()[:, 0], want), (name, n)


def _small_key_pairs(api, ctx, n, seed):
    """n (sig, msg) that ed25519_Verify_Check accepts under the small-order key t*T8 of `ctx`: R = S*B + j*T8 with j chosen so that the
    cofactorless equation holds, R itself not of small order -- the pairs only rule 3 rejects"""
    import hashlib
    import random
    rnd = random.Random(seed)
    T8 = sc.ed_order8_point()
    Ab = ctx[:32].tobytes()
    t = next(k for e, k in sc.small_order_encodings() if e == Ab)
    sigs, msgs = [], []
    while len(sigs) < n:
        S = rnd.getrandbits(252) % L
        SB = sc.ed_mul(S, sc.ED_B)
        m = rnd.getrandbits(256).to_bytes(32, "little")
        for j in range(8):
            Rb = sc.ed_enc(sc.ed_add(SB, sc.ed_mul(j, T8)))
            h = int.from_bytes(hashlib.sha512(Rb + Ab + m).digest(), "little") % L
            if (j + h * t) % 8 == 0 or (j - h * t) % 8 == 0:                    # the key is t*T8; both sign conventions go in
                sigs.append(np.frombuffer(Rb + S.to_bytes(32, "little"), np.uint8))
                msgs.append(np.frombuffer(m, np.uint8))
    sig, msg = np.stack(sigs[:4 * n]), np.stack(msgs[:4 * n])
    keep = api.ed25519_Verify_Check(ctx, sig, msg) == 1
    return sig[keep][:n], msg[keep][:n]


def test_verify_check_strict_on_two_streams_of_one_thread(api, oracle):
    """per-wave sizes, two streams of one thread, contexts of different classes in turn: a small-order key whose pairs the plain call
    accepts (strict: all 0) beside an honest key (strict: mostly 1) -- no call may take the other's key verdict"""
    import torch
    ctxs, priv, a, mixed_pk = _context_cases(api, oracle)
    ssig, smsg = _small_key_pairs(api, ctxs["small"], 48, 0x57AB)
    assert len(ssig) >= 24
    hsig, hmsg = _pairs(api, oracle, 700, priv, a, mixed_pk, "honest", 0x57AC)
    hwant = api.ed25519_Verify_Check_strict(ctxs["honest"], hsig, hmsg)
    assert hwant.sum() > 300 and not api.ed25519_Verify_Check_strict(ctxs["small"], ssig, smsg).any()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                # noqa: E731
    cases = [(dev(ctxs["small"][None, :]), dev(ssig), dev(smsg), np.zeros(len(ssig), np.int32)),
             (dev(ctxs["honest"][None, :]), dev(hsig), dev(hmsg), hwant),
             (dev(ctxs["small"][None, :]), dev(ssig[:1]), dev(smsg[:1]), np.zeros(1, np.int32)),
             (dev(ctxs["honest"][None, :]), dev(hsig[:1]), dev(hmsg[:1]), hwant[:1])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(25):
        outs = []
        for k, (c, s, m, _) in enumerate(cases):
            with torch.cuda.stream(streams[(k + rep) % 2]):
                out = torch.full((s.shape[0], 1), 7, dtype=torch.int32, device="cuda")
                api.ed25519_Verify_Check_strict_dev(out, c, s, m)
                outs.append(out)
        torch.cuda.synchronize()
        for k, (out, case) in enumerate(zip(outs, cases)):
            assert np.array_equal(out.cpu().numpy()[:, 0], case[3]), (rep, k)
