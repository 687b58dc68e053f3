"""Sizes, rows and the runner for the host-pointer (*_batch) calls cut into pipeline pieces (tests/test_gpu_batch_pieces.py runs them on
the device, tests/test_piece_cases.py checks on the CPU that the sizes and the rows are what that test's assertions rest on).  No GPU
in here: the expectations come from the big-integer models and the oracle, the runner is handed the loaded library.

run_batch (csrc/host_pipeline.hpp) cuts a call at 2^17 rows into pieces of piece_rows() rows, and any call at the staging cap of
256 MiB per buffer set.  A piece that is given the wrong count, the wrong staging pointer or an array of the wrong width puts rows
k * chunk places away from where they belong, so every call's rows repeat with a PERIOD that no such shift can hide: more than 24
rows (the most pieces of a call here) and coprime to both piece sizes, 5632 and 65 536 -- odd and no multiple of 11.  The models take
1 to 6 ms a row: `period` rows are modelled once per process, and cycled to n rows where the call is made."""
import collections
import functools
import math
import os

import numpy as np

FILL = 0xA5

# ---- sizes ---------------------------------------------------------------------------------------------------------------------
DEFAULT_N = (1 << 17) + 3                  # default knobs: 65 536 + 65 536 + 3 rows; the tail of 3 is a piece, not a zero-copy call
CUT_N = 131073                             # under CUT_KNOBS: 23 pieces of 5632 rows and one of 1537 -- three times the buffer sets
CUT_KNOBS = {"C25519_AMD_BATCH_PIECES": "24", "C25519_AMD_PIECE_MIN_ROWS": "256", "C25519_AMD_STAGERS": "3", "C25519_AMD_DRAINERS": "2"}
SMALL_N = 4097                             # the one-piece call made after the cut ones
PIECE_THRESHOLD = 1 << 17
STAGING_CAP = 256 << 20
MOST_PIECES = 24
PIECE_SIZES = (5632, 65536)


def round_up(x, a):
    return (x + a - 1) // a * a


def cap_rows(row):
    """the most rows of `row` bytes (all arrays of the call together) one buffer set stages"""
    return round_up(STAGING_CAP // (row or 1) + 1, 256)


def piece_rows(n, row, pieces=8, floor_rows=1 << 16):
    """piece_rows of csrc/host_pipeline.hpp, restated: n / pieces rounded up to 256 and not below the floor from 2^17 rows on,
    everything at once below, and never more than the cap"""
    chunk = n
    if n >= PIECE_THRESHOLD:
        chunk = max(round_up(-(-n // pieces), 256), floor_rows)
    return min(chunk, cap_rows(row))


def knob_values(env):
    """(pieces, floor_rows) as the library reads them from an environment"""
    def num(name):
        try:
            return int(env.get(name, "") or 0)
        except ValueError:
            return 0
    p, f = num("C25519_AMD_BATCH_PIECES"), num("C25519_AMD_PIECE_MIN_ROWS")
    return (p if 2 <= p <= 64 else 8), (f if f >= 256 else 1 << 16)


def split(n, row, env=None):
    """the piece sizes of a call of n rows of `row` bytes"""
    chunk = piece_rows(n, row, *knob_values(env or {}))
    return [min(chunk, n - lo) for lo in range(0, n, chunk)]


def period_ok(p):
    return p > MOST_PIECES and all(math.gcd(p, c) == 1 for c in PIECE_SIZES)


def usable_period(k):
    """the longest period of at most k rows that meets the condition"""
    p = next(p for p in range(k, MOST_PIECES, -1) if period_ok(p))
    return p


def shifts(period):
    """where a misplaced piece's rows come from, as distances mod period: k pieces of either size, and of the cap's"""
    return sorted({k * c % period for c in PIECE_SIZES + (cap_rows(CAP_MSG_SIZE + 32),) for k in range(1, MOST_PIECES)})


# ---- the staging cap: ed25519_HashToScalar_batch stages msg_size + 32 bytes a row ----------------------------------------------
# the shortest messages at which the cap is 4096 rows, of a length that is no multiple of 16 (so the second piece starts at a row that
# is not aligned in the caller's array), and five rows more than the cap: two pieces far below 2^17 rows
CAP_MSG_SIZE = next(m for m in range(1, 1 << 17) if m % 16 and cap_rows(m + 32) == 4096)
CAP_N = cap_rows(CAP_MSG_SIZE + 32) + 5
CAP_PERIOD = 29


# ---- calls -------------------------------------------------------------------------------------------------------------------------
# args, in the order of the C prototype:
#   ("out", key)   an output array; arrays[key] holds its expectation for the period rows (2-D uint8 rows, or 1-D int32 / uint32)
#   ("in", key)    an input array, arrays[key] cycled to n rows
#   ("size", key)  the row width of arrays[key] in bytes (msg_size, alpha_size)
#   ("bytes", key) a pointer to arrays[key] as it is (the DST, the signer contexts); ("len", key) its length in bytes, ("rows", key) in rows
#   ("val", v)     a number
#   ("n",)         the row count
Call = collections.namedtuple("Call", "symbol args label")


def call(symbol, *args, label=None):
    return Call(symbol, tuple(args), label or symbol)


O, I = (lambda k: ("out", k)), (lambda k: ("in", k))    # noqa: E731
N = ("n",)

_SCALAR_UNARY = {"Negate": "negate", "Complement": "complement"}
_SCALAR_BINARY = {"Add": "add", "Sub": "sub", "Mul": "mul"}

CALLS = {
    "keys": [
        call("ed25519_ClassifyKey_batch", O("flags"), I("pk"), N),
        call("ed25519_PublicKey_to_X25519_batch", O("xpk"), O("xpk_ok"), I("pk"), N),
        call("ed25519_PrivateKey_to_X25519_batch", O("xsk"), I("priv"), N),
    ],
    "group": [
        call("ed25519_ScalarMult_batch", O("q"), O("q_ok"), I("scalar"), I("point"), N),
        call("ed25519_ScalarMult_noclamp_batch", O("q_nc"), O("q_nc_ok"), I("scalar"), I("point"), N),
        call("ed25519_ScalarMultBase_batch", O("base"), I("scalar"), N),
        call("ed25519_ScalarMultBase_noclamp_batch", O("base_nc"), I("scalar"), N),
        call("ed25519_PointAdd_batch", O("sum"), O("sum_ok"), I("add_p"), I("add_q"), N),
        call("ed25519_PointSub_batch", O("diff"), O("diff_ok"), I("add_p"), I("add_q"), N),
    ],
    "ristretto255": [
        call("ristretto255_IsValidPoint_batch", O("valid"), I("any_point"), N),
        call("ristretto255_FromHash_batch", O("from_hash"), I("hash"), N),
        call("ristretto255_ScalarMult_batch", O("q"), O("q_ok"), I("scalar"), I("point"), N),
        call("ristretto255_ScalarMultBase_batch", O("base"), I("scalar"), N),
        call("ristretto255_PointAdd_batch", O("sum"), O("sum_ok"), I("add_p"), I("add_q"), N),
        call("ristretto255_PointSub_batch", O("diff"), O("diff_ok"), I("add_p"), I("add_q"), N),
    ],
    "scalar": [call("ed25519_ScalarReduce_batch", O("reduce"), I("w"), N)]
              + [call(f"ed25519_Scalar{k}_batch", O(v), I("x"), N) for k, v in _SCALAR_UNARY.items()]
              + [call(f"ed25519_Scalar{k}_batch", O(v), I("x"), I("y"), N) for k, v in _SCALAR_BINARY.items()]
              + [call("ed25519_ScalarMulAdd_batch", O("muladd"), I("x"), I("y"), I("z"), N),
                 call("ed25519_ScalarInvert_batch", O("recip"), O("ok"), I("x"), N),
                 call("ed25519_ScalarIsCanonical_batch", O("canonical"), I("x"), N)],
    "h2c": [
        call("c25519_ExpandMessageXmd_batch", O("xmd"), I("xmd_msg"), ("size", "xmd_msg"), ("bytes", "xmd_dst"), ("len", "xmd_dst"),
             ("val", 129), N),
        call("ed25519_MapToCurve_batch", O("map"), I("u"), N),
    ] + [call(sym, O(k), I(k + "_msg"), ("size", k + "_msg"), ("bytes", k + "_dst"), ("len", k + "_dst"), N)
         for sym, k in (("ed25519_HashToCurve_batch", "h2curve"), ("ed25519_EncodeToCurve_batch", "e2curve"),
                        ("ristretto255_HashToGroup_batch", "h2group"), ("ed25519_HashToScalar_batch", "h2scalar"))],
    "vrf": [
        call("ed25519_VRF_Prove_batch", O("pi_a"), I("priv_a"), I("alpha_a"), ("size", "alpha_a"), N, label="Prove, alpha of 51 bytes"),
        call("ed25519_VRF_Prove_batch", O("pi_b"), I("priv_b"), I("alpha_b"), ("size", "alpha_b"), N, label="Prove, alpha of 52 bytes"),
        call("ed25519_VRF_Verify_batch", O("beta_r"), O("ok_r"), I("pk_r"), I("pi_r"), I("alpha_r"), ("size", "alpha_r"), N,
             label="Verify, the rejection rows"),
        call("ed25519_VRF_Verify_batch", O("beta_v"), O("ok_v"), I("pk_v"), I("pi_v"), I("alpha_v"), ("size", "alpha_v"), N,
             label="Verify, alpha of 52 bytes"),
        call("ed25519_VRF_ProofToHash_batch", O("beta_h"), O("ok_h"), I("pi_r"), N),
    ],
    "sign_indexed": [
        call("ed25519_SignMessage_indexed_batch", O("sig"), ("bytes", "ctx"), ("rows", "ctx"), I("ctx_index"), I("msg"), ("size", "msg"), N),
    ],
}
FAMILIES = tuple(CALLS)

# the one-piece calls made after the cut ones, in the child process: both lanes' scratch slabs have been used and grown by then
SMALL_AFTER = {
    "group": [call("ed25519_ScalarMult_batch", O("q"), O("q_ok"), I("scalar"), I("point"), N, label="ScalarMult at 4097 rows, afterwards")],
    "keys": [call("ed25519_ScalarMult_batch", O("sm_q"), O("sm_q_ok"), I("sm_scalar"), I("sm_point"), N, label="ScalarMult at 4097 rows, afterwards"),
             call("ed25519_PublicKey_to_X25519_batch", O("xpk"), O("xpk_ok"), I("pk"), N, label="PublicKey_to_X25519 at 4097 rows, afterwards")],
}

CAP_CALL = call("ed25519_HashToScalar_batch", O("cap"), I("cap_msg"), ("size", "cap_msg"), ("bytes", "cap_dst"), ("len", "cap_dst"), N)


def in_place_variants(family):
    """[(call, output key, input key)]: every call of the family with a 32-byte-row output, once for each of its 32-byte-row inputs"""
    if family != "scalar":
        return []
    out = []
    for c in CALLS[family]:
        outs = [a[1] for a in c.args if a[0] == "out" and a[1] not in ("ok", "canonical")]
        ins = [a[1] for a in c.args if a[0] == "in" and a[1] != "w"]
        out += [(c, outs[0], k) for k in ins if outs]
    return out


def keys_of(c, kind):
    return [a[1] for a in c.args if a[0] == kind]


def row_bytes(a):
    return a.itemsize * int(np.prod(a.shape[1:], dtype=np.int64))


def staged_row(c, arrays):
    """bytes per row of all arrays the call stages: the `row` of piece_rows"""
    return sum(row_bytes(arrays[k]) for k in keys_of(c, "in") + keys_of(c, "out"))


def period_of(c, arrays):
    lengths = {len(arrays[k]) for k in keys_of(c, "in") + keys_of(c, "out")}
    assert len(lengths) == 1, (c.label, lengths)
    return lengths.pop()


# ---- rows ------------------------------------------------------------------------------------------------------------------------
def _rows(rows, width):
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]).reshape(len(rows), width).copy()


def _seeded(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _dst(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _period_rows(*inputs):
    """the inputs of one call without repeated rows (a model's case set may name a value twice), cut to the longest usable period"""
    seen, keep = set(), []
    for i in range(len(inputs[0])):
        row = tuple(a[i].tobytes() for a in inputs)
        if row not in seen:
            seen.add(row)
            keep.append(i)
    keep = keep[:usable_period(len(keep))]
    return [a[keep] for a in inputs]


def _scalarmult_rows(prefix=""):
    import group_model
    sc, pt = _period_rows(*group_model.case_set()[:2])
    q, ok = group_model.expected_scalarmult(sc, pt, True)
    return {prefix + "scalar": sc, prefix + "point": pt, prefix + "q": q, prefix + "q_ok": ok}


def _keys():
    import key_model
    # five keys of every label: the model walks every key by L with affine additions, 0.1 s a key
    keys, labels = key_model.case_set()
    taken, keep = collections.Counter(), []
    for i, lab in enumerate(labels):
        taken[lab] += 1
        if taken[lab] <= 5:
            keep.append(i)
    keys, = _period_rows(keys[keep])
    flags, xpk, ok = key_model.expected(keys)
    priv = _seeded((251, 64), 0x91EC01)
    xsk = _rows([key_model.private_to_x25519(bytes(r)) for r in priv], 32)
    return dict(pk=keys, flags=flags, xpk=xpk, xpk_ok=ok, priv=priv, xsk=xsk, **_scalarmult_rows("sm_"))


def _group():
    import group_model
    out = _scalarmult_rows()
    sc, pt = out["scalar"], out["point"]
    out["q_nc"], out["q_nc_ok"] = group_model.expected_scalarmult(sc, pt, False)
    out["base"], out["base_nc"] = group_model.expected_base(sc, True), group_model.expected_base(sc, False)
    p, q = _period_rows(*group_model.add_cases()[:2])
    out["add_p"], out["add_q"] = p, q
    out["sum"], out["sum_ok"] = group_model.expected_add(p, q, False)
    out["diff"], out["diff_ok"] = group_model.expected_add(p, q, True)
    return out


def _ristretto255():
    import ristretto_model as rm
    sc, pt = _period_rows(*rm.case_set()[:2])
    out = dict(scalar=sc, point=pt, base=rm.expected_base(sc))
    out["q"], out["q_ok"] = rm.expected_scalarmult(sc, pt)
    anyp, = _period_rows(rm.points()[0])
    out["any_point"], out["valid"] = anyp, rm.expected_valid(anyp)
    h, = _period_rows(rm.hashes())
    out["hash"], out["from_hash"] = h, rm.expected_from_hash(h)
    p, q = _period_rows(*rm.add_cases()[:2])
    out["add_p"], out["add_q"] = p, q
    out["sum"], out["sum_ok"] = rm.expected_add(p, q, False)
    out["diff"], out["diff_ok"] = rm.expected_add(p, q, True)
    return out


def _scalar():
    import scalar_model
    cs = scalar_model.case_set()
    k = usable_period(len(cs["w"]))                      # 1034 rows: one too many
    out = {name: a for name, a in cs.items() if name not in ("w", "reduce")}
    out["w"], out["reduce"] = cs["w"][:k], cs["reduce"][:k]
    return out


# the hashing calls: (DST length, message length); msg_size + dst_len + 4 mod 128 is the place in the padding's block -- 127, 0, 112 and 1
# sit on both sides of its edge.  235, 190 and 237 are no multiples of 4: a piece's rows start at an odd place in the staging buffer.
H2C_SHAPES = {"h2curve": (16, 235), "e2curve": (62, 190), "h2group": (255, 237), "h2scalar": (1, 252), "xmd": (45, 7)}
H2C_SLOW_PERIOD, H2C_FAST_PERIOD = 53, 251               # three maps and a cofactor walk a row against hashlib alone


def _h2c():
    import h2c_model as hm
    assert all(d in hm.DST_LENGTHS for d, _ in H2C_SHAPES.values())
    out = {}
    for key, (dst_len, msg_size) in H2C_SHAPES.items():
        fast = key in ("xmd", "h2scalar")
        msgs = _seeded((H2C_FAST_PERIOD if fast else H2C_SLOW_PERIOD, msg_size), 0x91EC10 + msg_size)
        dst = hm.make_dst(dst_len)
        name = {"h2curve": "hash_to_curve", "e2curve": "encode_to_curve", "h2group": "hash_to_group", "h2scalar": "hash_to_scalar", "xmd": "xmd"}[key]
        out[key + "_msg"], out[key + "_dst"] = msgs, _dst(dst)
        out[key] = hm.expected(name, dst, msgs, 129 if key == "xmd" else None)
    k = usable_period(len(hm.map_inputs()))
    out["u"], out["map"] = hm.map_inputs()[:k], hm.expected_map()[:k]
    return out


VRF_ALPHAS = (51, 52)                                    # 32 + alpha + 40 + 4 = 127 and 0 mod 128: the last byte of a block, and a full one
VRF_PERIOD = 53


def _vrf_honest(alpha_len):
    import vrf_model as vm
    privs = [vm.private_key(vm._bytes(32, f"piece seed {alpha_len} {j}")) for j in range(VRF_PERIOD)]
    alphas = [vm._bytes(alpha_len, f"piece alpha {alpha_len} {j}") for j in range(VRF_PERIOD)]
    return privs, alphas, [vm.prove(p, a) for p, a in zip(privs, alphas)]


def _vrf():
    import vrf_model as vm
    assert all(a in vm.ALPHA_LENGTHS for a in VRF_ALPHAS) and vm.REJECT_ALPHA % 4
    out = {}
    for tag, alpha_len in zip("ab", VRF_ALPHAS):
        privs, alphas, pis = _vrf_honest(alpha_len)
        out["priv_" + tag], out["alpha_" + tag], out["pi_" + tag] = _rows(privs, 64), _rows(alphas, alpha_len), _rows(pis, vm.PROOF_SIZE)
    r = vm.rejections()
    out.update(pk_r=r["pk"], pi_r=r["pi"], alpha_r=r["alpha"], ok_r=r["ok"], beta_r=r["beta"], ok_h=r["ok_hash"], beta_h=r["beta_hash"])
    # the honest rows of the second length through Verify, a bit of s flipped in every third proof
    pi_v = out["pi_b"].copy()
    pi_v[1::3, 50] ^= 0x10
    pk_v = out["priv_b"][:, 32:].copy()
    ver = [vm.verify(bytes(k), bytes(p), bytes(a)) for k, p, a in zip(pk_v, pi_v, out["alpha_b"])]
    out.update(pk_v=pk_v, pi_v=pi_v, alpha_v=out["alpha_b"], beta_v=_rows([v[0] for v in ver], vm.OUTPUT_SIZE),
               ok_v=np.array([v[1] for v in ver], np.int32))
    return out


SIGN_CONTEXTS, SIGN_PERIOD, SIGN_MSG_SIZE = 7, 251, 47   # 47: the last one-block message of H(enc(R) || pk || m), and no multiple of 4


def _sign_indexed():
    import sign_ctx_model
    from oracle_lib import Oracle
    oracle = Oracle()
    _, priv = oracle.ed25519_keypair(_seeded((SIGN_CONTEXTS, 32), 0x91EC20))
    ctx = _rows([sign_ctx_model.sign_ctx(bytes(p)) for p in priv], 128)
    idx = np.random.default_rng(0x91EC21).integers(0, SIGN_CONTEXTS, SIGN_PERIOD).astype(np.uint32)
    msg = _seeded((SIGN_PERIOD, SIGN_MSG_SIZE), 0x91EC22)
    return dict(ctx=ctx, ctx_index=idx, msg=msg, sig=oracle.ed25519_sign(priv[idx], msg))


_BUILDERS = {"keys": _keys, "group": _group, "ristretto255": _ristretto255, "scalar": _scalar, "h2c": _h2c, "vrf": _vrf,
             "sign_indexed": _sign_indexed}


@functools.lru_cache(maxsize=None)
def family_rows(family):
    """{key: array}: the period rows of every input of the family's calls and the models' outputs for them, computed once per
    process and never written (the arrays are read-only)"""
    out = {k: np.ascontiguousarray(a) for k, a in _BUILDERS[family]().items()}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cap_rows_set():
    """the rows of the staging-cap call: CAP_PERIOD distinct messages of CAP_MSG_SIZE bytes and h2c_model.hash_to_scalar of each"""
    import h2c_model as hm
    dst = hm.make_dst(16)
    msgs = _seeded((CAP_PERIOD, CAP_MSG_SIZE), 0x91EC30)
    want = _rows([hm.hash_to_scalar(bytes(m), dst) for m in msgs], 32)
    out = dict(cap_msg=msgs, cap_dst=_dst(dst), cap=want)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the runner: one call through the C ABI on buffers it owns ---------------------------------------------------------------------
def run_call(lib, c, arrays, n, env=None, alias=None):
    """One call of n rows: the inputs are arrays[key] cycled to n rows, the outputs n + 1 rows of 0xA5 bytes.  Returns a dict that
    json can carry: the return code, how many rows differ from the cycled expectation, the first of them with the piece each falls
    in, whether the guard rows and the inputs survived.  alias = (output key, input key): that output is written over that input."""
    import ctypes as C
    env = os.environ if env is None else env
    period = period_of(c, arrays)
    idx = np.arange(n) % period
    chunk = piece_rows(n, staged_row(c, arrays), *knob_values(env))
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ins, outs, cargs = {}, {}, []
    shared = None
    if alias:
        shared = np.full((n + 1,) + arrays[alias[1]].shape[1:], FILL, arrays[alias[1]].dtype)
        shared[:n] = arrays[alias[1]][idx]
    for kind, *rest in c.args:
        key = rest[0] if rest else None
        if kind == "in":
            if key not in ins:
                ins[key] = shared if alias and key == alias[1] else np.ascontiguousarray(arrays[key][idx])
            cargs.append(ptr(ins[key]))
        elif kind == "out":
            want = arrays[key]
            if alias and key == alias[0]:
                outs[key] = shared
            else:
                outs[key] = np.full((n + 1) * row_bytes(want), FILL, np.uint8).view(want.dtype).reshape((n + 1,) + want.shape[1:])
            cargs.append(ptr(outs[key]))
        elif kind == "size":
            cargs.append(row_bytes(arrays[key]))
        elif kind == "bytes":
            cargs.append(ptr(arrays[key]))
        elif kind == "len":
            cargs.append(arrays[key].nbytes)
        elif kind == "rows":
            cargs.append(len(arrays[key]))
        elif kind == "val":
            cargs.append(key)
        else:
            cargs.append(n)
    rc = getattr(lib, c.symbol)(*cargs)
    res = dict(call=c.label + (f", {alias[0]} over {alias[1]}" if alias else ""), n=n, chunk=chunk, rc=rc, differ=0, first=[], guard=True,
               inputs_unchanged=True, error="")
    if rc:
        res["error"] = lib.c25519_amd_last_error().decode(errors="replace")
    for key, buf in outs.items():
        want = arrays[key][idx]
        diff = buf[:n] != want
        bad = np.flatnonzero(diff.any(axis=1) if diff.ndim > 1 else diff)
        res["differ"] += int(len(bad))
        res["first"] += [[key, int(i), int(i // chunk)] for i in bad[:4]]
        res["guard"] = res["guard"] and bool((buf[n:].view(np.uint8) == FILL).all())
    for key, buf in ins.items():
        if not (alias and key == alias[1]):
            res["inputs_unchanged"] = res["inputs_unchanged"] and bool(np.array_equal(buf, arrays[key][idx]))
    return res


def run_family(lib, family, arrays, n, env=None, small_after=False):
    """every call of the family at n rows, the in-place forms of the scalar calls, and (small_after) the one-piece calls behind them"""
    out = [run_call(lib, c, arrays, n, env) for c in CALLS[family]]
    out += [run_call(lib, c, arrays, n, env, alias=(o, i)) for c, o, i in in_place_variants(family)]
    if small_after:
        out += [run_call(lib, c, arrays, SMALL_N, env) for c in SMALL_AFTER.get(family, [])]
    return out


def failures(results):
    """the results that are not clean: a return code, a differing row, a written guard row or a changed input"""
    return [r for r in results if r["rc"] != 0 or r["differ"] or not r["guard"] or not r["inputs_unchanged"]]
