"""GPU suite: the base calls -- X25519, public keys, key pairs, signatures (blinded or not), verification -- at the sizes where
their DEFAULT dispatch changes form, byte for byte against the oracle, with every tunable unset.  At a threshold T the form below
runs its largest grid; at T + 1 the form above runs its smallest, with one element in its last wave, quad or workgroup.  Each case
also pins the form itself through c25519_amd_last_shape(): both forms give the same bytes, so a moved default would otherwise go
unseen.  Inputs: tests/dispatch_cases.py (checked on the CPU by tests/test_dispatch_cases.py).

The expected shapes are written out below as data, read off the thresholds and the figures they cite:
  engine_common.cuh   x25519_two_waves_for 512 (profiles/r05_small_batch_sweep.txt), x25519_quad_for 3584 .. 2^15, fixed_base_quad_for
                      1024 .. 2^14, verify_quad_for 1024 .. 2^15 (profiles/r06_mid_batch_sweep.txt), fixed_base_coop_for 2048
                      (profiles/r04_small_batch_sweep.txt; it decides for the blinded calls, which have no quad form)
  engine_x25519.hip   x25519_split_for 2^16 (two launches beyond), x25519_block_for 64 lanes up to 2^16 (profiles/r03_batch_sweep.txt)
  engine_fixed_base.hip  the one-lane kernels over the wide comb, the default (profiles/r05_ab_base_comb.txt), run 256-lane workgroups at
                      every size; 256 / 512 / 1024 lanes by n (bm_block_for) are the shapes of the LDS comb, BASE_COMB = 0, which
                      test_blinded_calls_over_the_lds_comb forces -- the one test here that sets a tunable."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dispatch_cases as dc
from curve25519_amd import synth
from dispatch_cases import THREADS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (form, lanes per workgroup): 1 one element per workgroup, 2 four lanes per element, 3 one lane per element (X25519: one launch),
# 4 one lane per element and the shared inversion as a launch of its own
PER_WAVE, TWO_WAVES, THREE_WAVES, SIGN_WAVES = (1, 64), (1, 128), (1, 192), (1, 128)
QUAD, VERIFY_QUAD = (2, 64), (2, 256)
LANE_X25519, LANE_VERIFY = (3, 64), (3, 256)
SPLIT = (4, 256)

X25519_SHAPES = {512: TWO_WAVES, 513: PER_WAVE, 3584: PER_WAVE, 3585: QUAD, 32768: QUAD, 32769: LANE_X25519, 65536: LANE_X25519,
                 65537: SPLIT}
LADDER_PUBLIC_SHAPES = {512: PER_WAVE, 513: PER_WAVE, 3584: PER_WAVE, 3585: QUAD, 32768: QUAD, 32769: LANE_X25519}
FAST_PUBLIC_SHAPES = {512: PER_WAVE, 513: PER_WAVE, 3584: QUAD, 3585: QUAD, 32768: SPLIT, 32769: SPLIT}
KEYPAIR_SHAPES = {1024: PER_WAVE, 1025: QUAD, 16384: QUAD, 16385: SPLIT}
SIGN_SHAPES = {1024: SIGN_WAVES, 1025: QUAD, 16384: QUAD, 16385: SPLIT}
BLINDED_KEYPAIR_SHAPES = {2: PER_WAVE, 65: PER_WAVE, 2048: PER_WAVE, 2049: SPLIT, 65537: SPLIT, 131073: SPLIT}
BLINDED_SIGN_SHAPES = {2: SIGN_WAVES, 65: SIGN_WAVES, 2048: SIGN_WAVES, 2049: SPLIT, 65537: SPLIT, 131073: SPLIT}
VERIFY_SHAPES = {1024: THREE_WAVES, 1025: VERIFY_QUAD, 32768: VERIFY_QUAD, 32769: LANE_VERIFY}
# the LDS comb (BASE_COMB = 0) has no per-wave form for a blinded call: one lane per element at every size, workgroups by n
LDS_COMB_BLINDED_SHAPES = {2049: (4, 256), 65536: (4, 256), 65537: (4, 512), 131072: (4, 512), 131073: (4, 1024)}
# a *_batch call: the form of the whole call's size, whatever its pieces are
BATCH_SHAPES = {"shared": {32769: LANE_X25519, 131073: SPLIT}, "ladder_public": {32769: LANE_X25519, 131073: SPLIT},
                "fast_public": {32769: SPLIT, 131073: SPLIT}, "keypair": {32769: SPLIT, 131073: SPLIT},
                "sign": {32769: SPLIT, 131073: SPLIT}, "verify": {32769: LANE_VERIFY, 131073: LANE_VERIFY}}

DISPATCH_TUNABLES = ("COOP_MAX", "QUAD_MIN", "QUAD_MAX", "LADDER2_MAX", "XF_SPLIT", "BASE_COMB")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(autouse=True)
def defaults_only(api):
    from curve25519_amd import _lib
    L = _lib.load()
    for name in DISPATCH_TUNABLES:
        assert L.c25519_amd_tunable_get(name.encode()) == -1, f"{name} is set: these tests pin the DEFAULT dispatch"
    yield
    for name in DISPATCH_TUNABLES:
        assert L.c25519_amd_tunable_get(name.encode()) == -1, name


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def empty(n, width, dtype=None):
    import torch
    return torch.empty((n, width), dtype=dtype or torch.uint8, device=torch.device("cuda", 0))


def host(t):
    return t.cpu().numpy()


def test_last_shape_is_per_thread_and_cleared_by_release(api):
    import threading
    from curve25519_amd import _lib
    L = _lib.load()
    sk = synth.random_bytes((3, 32), 0xD1)
    api.curve25519_dh_CalculatePublicKey(sk)
    assert api.last_shape() == PER_WAVE
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.c25519_amd_last_shape()))
    t.start()
    t.join()
    assert seen == [-1]                                                # another thread has made no base call
    api.ed25519_CreateKeyPair(sk)
    api.ed25519_SignMessage(np.zeros((3, 64), np.uint8), np.zeros((3, 5), np.uint8))
    assert api.last_shape() == SIGN_WAVES and L.c25519_amd_last_shape() == 1 | 128 << 8
    L.c25519_amd_thread_release()
    assert L.c25519_amd_last_shape() == -1 and api.last_shape() is None


@pytest.mark.parametrize("n", dc.X25519_SIZES)
def test_x25519_shared_key(api, oracle, n):
    pk_np, sk_np, low = dc.x25519_rows(n)
    e_shared, e_clamped = oracle.x25519_shared(pk_np, sk_np, threads=THREADS)
    shared, pk, sk = empty(n, 32), up(pk_np), up(sk_np)
    api.curve25519_dh_CreateSharedKey_dev(shared, pk, sk)
    assert api.last_shape() == X25519_SHAPES[n]
    got = host(shared)
    assert np.array_equal(got, e_shared) and np.array_equal(host(sk), e_clamped)
    assert int((~got.any(axis=1)).sum()) == low                         # the low-order peers, the lone last row among them at some sizes


@pytest.mark.parametrize("n", dc.PUBLIC_KEY_SIZES)
def test_x25519_public_key_ladder_and_fixed_base(api, oracle, n):
    _, sk_np, _ = dc.x25519_rows(n)
    base = np.zeros((n, 32), np.uint8)
    base[:, 0] = 9
    e_pk, e_clamped = oracle.x25519_shared(base, sk_np, threads=THREADS)
    ladder, fast, sk1, sk2 = empty(n, 32), empty(n, 32), up(sk_np), up(sk_np)
    api.curve25519_dh_CalculatePublicKey_dev(ladder, sk1)
    assert api.last_shape() == LADDER_PUBLIC_SHAPES[n]
    api.curve25519_dh_CalculatePublicKey_dev(fast, sk2, fast=True)
    assert api.last_shape() == FAST_PUBLIC_SHAPES[n]
    assert np.array_equal(host(ladder), host(fast)) and np.array_equal(host(sk1), host(sk2))
    assert np.array_equal(host(ladder), e_pk) and np.array_equal(host(sk1), e_clamped)


@pytest.mark.parametrize("n", dc.FIXED_BASE_SIZES)
def test_key_pair_and_signature(api, oracle, n):
    sk_np, _ = dc.sign_rows(n, 0)
    e_pub, e_priv = oracle.ed25519_keypair(sk_np, threads=THREADS)
    pub, priv = empty(n, 32), empty(n, 64)
    api.ed25519_CreateKeyPair_dev(pub, priv, up(sk_np))
    assert api.last_shape() == KEYPAIR_SHAPES[n]
    assert np.array_equal(host(pub), e_pub) and np.array_equal(host(priv), e_priv)
    for mlen in dc.FIXED_BASE_LENGTHS[n]:
        _, msg_np = dc.sign_rows(n, mlen)
        sig = empty(n, 64)
        api.ed25519_SignMessage_dev(sig, priv, up(msg_np))
        assert api.last_shape() == SIGN_SHAPES[n], mlen
        assert np.array_equal(host(sig), oracle.ed25519_sign(e_priv, msg_np, threads=THREADS)), mlen


def blinding_context(seed=b"dispatch edges"):
    """one 192-byte context from ed25519_Blinding_Init, on the host and on the device"""
    from curve25519_amd import _lib
    L = _lib.load()
    ctx = np.zeros(192, np.uint8)
    sbuf = np.frombuffer(seed, np.uint8).copy()
    assert L.ed25519_Blinding_Init(ctx.ctypes.data, sbuf.ctypes.data, len(seed)) == ctx.ctypes.data
    assert ctx[:32].any() and ctx[32:64].any()
    return up(ctx.reshape(1, 192))


def blinded_calls(api, oracle, n, lengths, keypair_shape, sign_shape, comb=None):
    """the blinded key pair and signatures of n elements (with BASE_COMB = comb where given) against the DEFAULT unblinded calls'
    bytes, and against the oracle's: every row up to ORACLE_MAX_BLINDED elements, the first and last 64 rows beyond"""
    import contextlib
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    forced = (lambda: _lib.tunable("BASE_COMB", comb)) if comb is not None else contextlib.nullcontext
    rows = np.arange(n) if n <= dc.ORACLE_MAX_BLINDED else np.r_[0:64, n - 64:n]
    ctx = blinding_context()
    sk_np, _ = dc.sign_rows(n, 0)
    sk = up(sk_np)
    pub, priv, bpub, bpriv = empty(n, 32), empty(n, 64), empty(n, 32), empty(n, 64)
    api.ed25519_CreateKeyPair_dev(pub, priv, sk)
    with forced():
        _lib.check(L.ed25519_CreateKeyPair_blinded_dev(P(bpub), P(bpriv), P(ctx), P(sk), n, st), "ed25519_CreateKeyPair_blinded_dev")
        assert api.last_shape() == keypair_shape
    assert torch.equal(bpub, pub) and torch.equal(bpriv, priv)
    e_pub, e_priv = oracle.ed25519_keypair(np.ascontiguousarray(sk_np[rows]), threads=THREADS)
    assert np.array_equal(host(bpub)[rows], e_pub) and np.array_equal(host(bpriv)[rows], e_priv)
    for mlen in lengths:
        _, msg_np = dc.sign_rows(n, mlen)
        msg, sig, bsig = up(msg_np), empty(n, 64), empty(n, 64)
        api.ed25519_SignMessage_dev(sig, priv, msg)
        with forced():
            _lib.check(L.ed25519_SignMessage_blinded_dev(P(bsig), P(priv), P(ctx), P(msg), mlen, n, st), "ed25519_SignMessage_blinded_dev")
            assert api.last_shape() == sign_shape, mlen
        assert torch.equal(bsig, sig), mlen
        assert np.array_equal(host(bsig)[rows], oracle.ed25519_sign(e_priv, np.ascontiguousarray(msg_np[rows]), threads=THREADS)), mlen


@pytest.mark.parametrize("n", dc.BLINDED_SIZES)
def test_blinded_key_pair_and_signature(api, oracle, n):
    blinded_calls(api, oracle, n, dc.BLINDED_LENGTHS[n], BLINDED_KEYPAIR_SHAPES[n], BLINDED_SIGN_SHAPES[n])


@pytest.mark.parametrize("n", sorted(LDS_COMB_BLINDED_SHAPES))
def test_blinded_calls_over_the_lds_comb(api, oracle, n):
    """BASE_COMB = 0 around the blinded calls, the only tunable this module sets: the blinded one-lane kernels in the 512- and
    1024-lane workgroups that only the LDS comb runs (the default, the wide comb, stays at 256 lanes), at both sides of
    bm_block_for's 2^16 and 2^17"""
    shape = LDS_COMB_BLINDED_SHAPES[n]
    blinded_calls(api, oracle, n, dc.MSG_LENGTHS[n % 2::2], shape, shape, comb=0)


@pytest.mark.parametrize("n,mlen", [(n, mlen) for n in dc.VERIFY_SIZES for mlen in dc.VERIFY_LENGTHS[n]])
def test_verification(api, oracle, n, mlen):
    from curve25519_amd import _lib
    import torch
    sig_np, pk_np, msg_np, bad_row = dc.verify_rows(oracle, n, mlen)
    exp = oracle.ed25519_verify(sig_np, pk_np, msg_np, threads=THREADS)
    ok = empty(n, 1, torch.int32)
    api.ed25519_VerifySignature_dev(ok, up(sig_np), up(pk_np), up(msg_np))
    assert api.last_shape() == VERIFY_SHAPES[n]
    got = host(ok).reshape(-1)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:16]
    assert exp[n - dc.TAIL:].any() and not exp[n - dc.TAIL:].all() and exp[bad_row] == 0
    assert _lib.load().c25519_amd_verify_last_slow_elements() >= 1      # the undecodable key of the tail went through the slow list


BATCH_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r)
from curve25519_amd import api
d = np.load(sys.argv[1])
out, shapes = {}, {}
for n in (%d, %d):
    s = lambda k: d["%%s_%%d" %% (k, n)]
    out["shared_%%d" %% n], out["clamped_%%d" %% n] = api.curve25519_dh_CreateSharedKey(s("pk"), s("sk"))
    shapes["shared_%%d" %% n] = api.last_shape()
    out["ladder_%%d" %% n], _ = api.curve25519_dh_CalculatePublicKey(s("sk"))
    shapes["ladder_public_%%d" %% n] = api.last_shape()
    out["fast_%%d" %% n], _ = api.curve25519_dh_CalculatePublicKey(s("sk"), fast=True)
    shapes["fast_public_%%d" %% n] = api.last_shape()
    out["pub_%%d" %% n], out["priv_%%d" %% n] = api.ed25519_CreateKeyPair(s("esk"))
    shapes["keypair_%%d" %% n] = api.last_shape()
    out["sig_%%d" %% n] = api.ed25519_SignMessage(out["priv_%%d" %% n], s("msg"))
    shapes["sign_%%d" %% n] = api.last_shape()
    out["ok_%%d" %% n] = api.ed25519_VerifySignature(s("vsig"), s("vpk"), s("vmsg"))
    shapes["verify_%%d" %% n] = api.last_shape()
np.savez(sys.argv[2], **out)
print(json.dumps(shapes))
"""


def test_host_pointer_calls_report_the_whole_calls_form(api, oracle):
    """The *_batch forms in a fresh process with C25519_AMD_BATCH_PIECES = 24 (and pieces allowed down to 256 rows): one call of
    each operation at 32769 -- which the pipeline never cuts, whatever BATCH_PIECES says: it cuts from 2^17 rows on -- and one at
    131073, which it cuts into 23 pieces of 5632 rows and one of 1537.  A piece of 5632 alone would run on quads, 1537 X25519 elements
    one per wave: the call must report the form of ITS size (host_pipeline.hpp: batch_shape_hint), and give the same bytes."""
    import json
    small, big = dc.BATCH_SIZE, 131073
    mlen = {small: 176, big: 47}
    data, want = {}, {}
    for n in (small, big):
        pk, sk, _ = dc.x25519_rows(n)
        esk, msg = dc.sign_rows(n, mlen[n])
        shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
        ladder, _ = api.curve25519_dh_CalculatePublicKey(sk)
        fast, _ = api.curve25519_dh_CalculatePublicKey(sk, fast=True)
        pub, priv = api.ed25519_CreateKeyPair(esk)
        sig = api.ed25519_SignMessage(priv, msg)
        if n == small:                                                  # (these rows against the oracle: test_x25519_shared_key, test_verification)
            vsig, vpk, vmsg, _ = dc.verify_rows(oracle, n, mlen[n])
            e_pub, e_priv = oracle.ed25519_keypair(esk, threads=THREADS)
            assert np.array_equal(pub, e_pub) and np.array_equal(priv, e_priv)
            assert np.array_equal(sig, oracle.ed25519_sign(e_priv, msg, threads=THREADS))
            ok = api.ed25519_VerifySignature(vsig, vpk, vmsg)
            assert ok[n - dc.TAIL:].any() and not ok[n - dc.TAIL:].all()
        else:
            vsig, vmsg, bad = synth.corrupt_for_verify(sig, msg)
            vpk = pub.copy()
            vpk[n - 1] = dc.undecodable_key(0xD1620000)
            ok = api.ed25519_VerifySignature(vsig, vpk, vmsg)
            assert np.array_equal(ok[:n - 1] == 0, bad[:n - 1]) and ok[n - 1] == 0
        assert np.array_equal(ladder, fast)
        for k, v in (("pk", pk), ("sk", sk), ("esk", esk), ("msg", msg), ("vsig", vsig), ("vpk", vpk), ("vmsg", vmsg)):
            data[f"{k}_{n}"] = v
        for k, v in (("shared", shared), ("clamped", clamped), ("ladder", ladder), ("fast", fast), ("pub", pub), ("priv", priv),
                     ("sig", sig), ("ok", ok)):
            want[f"{k}_{n}"] = v
    env = {**os.environ, "C25519_AMD_BATCH_PIECES": "24", "C25519_AMD_PIECE_MIN_ROWS": "256"}
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), **data)
        p = subprocess.run([sys.executable, "-c", BATCH_CHILD % (ROOT, small, big), os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")],
                           capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out = np.load(os.path.join(tmp, "out.npz"))
        for name, v in want.items():
            assert np.array_equal(out[name], v), name
    shapes = json.loads(p.stdout.strip().splitlines()[-1])
    for op, by_size in BATCH_SHAPES.items():
        for n, shape in by_size.items():
            assert tuple(shapes[f"{op}_{n}"]) == shape, (op, n)
