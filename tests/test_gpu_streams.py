"""GPU suite (MI355X): the *_dev calls issued from ONE thread on several streams, with the thread's kept device state in flight.

The calls are asynchronous, and some of what they leave on the device belongs to the thread and not to the stream: the work slabs
(four per device, a further stream takes over the least recently used one), the kept buffer with the comb of the last big
one-key verification (KEEP_VERIFY), the one with the comb of the last big one-peer X25519 call (KEEP_PEER), and what the three
last-call hooks read.  Here a call walks key 0's comb on one stream while the call that rebuilds the buffer for key 1 is enqueued
on another, without any synchronisation in between; every result is compared byte for byte with the oracle's
(tests/stream_cases.py, checked on the CPU by tests/test_stream_cases.py).

Each scenario runs twice: with the path hook read after every call (the hook synchronises: this run shows which path decided each
call, and that the combs were walked at all), and with nothing but the calls between the first and the last (only this run can
see a missing wait between streams).  Correct code passes both whatever the timing."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

FILL = 0xA5
SEED = bytes(range(32))
MODES = pytest.mark.parametrize("hooks", (True, False), ids=("hooks_read", "no_sync"))


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def streams(api):
    import torch
    return [torch.cuda.Stream(dev()) for _ in range(6)]


def dev():
    import torch
    return torch.device("cuda", 0)


def up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev())     # (a copy: the case arrays are read-only)


def host(t):
    return t.cpu().numpy()


def filled(rows, width, dtype=None):
    """a device tensor of `rows` rows of `width` bytes, every byte FILL: a result that is never written does not pass"""
    import torch
    t = torch.full((rows, width), FILL, dtype=torch.uint8, device=dev())
    return t if dtype is None else t.view(dtype)


def verdicts(rows):
    import torch
    return filled(rows, 4, torch.int32)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def cur():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def release():
    _lib.load().c25519_amd_thread_release()


def fresh_thread_state(api, streams, one_peer):
    """nothing remembered from the test before (c25519_amd_thread_release), then a work slab for each of the scenario's streams: a
    plain X25519 call a little larger than the largest call to come, so that the calls of the scenario find their slab and only
    enqueue -- a call that has to allocate one first may reach the device when the call before it has finished there"""
    import torch
    release()
    n = one_peer["sk"].shape[0]
    pk = one_peer["sk"]                                     # (any 32-byte rows serve as keys here)
    for st in streams[:3]:
        with torch.cuda.stream(st):
            api.curve25519_dh_CreateSharedKey_dev(filled(n, 32), pk, pk.clone())
    torch.cuda.synchronize()


def check_hook():
    return _lib.load().c25519_amd_verify_check_last_wide()


def peer_hook():
    return _lib.load().c25519_amd_x25519_one_peer_last_wide()


def slow_hook():
    return _lib.load().c25519_amd_verify_last_slow_elements()


# ---- device copies of the inputs, made once -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_key(api, oracle):
    """per key: Verify_Init's context, the block tiled to the largest call under that key, the verdicts"""
    import torch
    out = []
    for k, (pub, sig, msg, ok) in enumerate(sc.one_key_sets(oracle)):
        rows = max(n for key, n in sc.VERIFY_CALLS.values() if key == k)
        ctx = api.ed25519_Verify_Init(pub)
        out.append(dict(ctx=up(ctx.reshape(1, 2080)), sig=up(sc.tile(sig, rows)), msg=up(sc.tile(msg, rows)), ok=sc.tile(ok, rows)))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def one_peer(api, oracle):
    import torch
    sk, peers = sc.one_peer_sets(oracle)
    rows = max(n for _, n in sc.PEER_CALLS.values()) + 64    # (+ 64: fresh_thread_state's slabs hold every call to come)
    out = {name: dict(pk=up(pk), shared=shared, clamped=clamped) for name, (pk, shared, clamped) in peers.items()}
    out["sk"] = up(sc.tile(sk, rows))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def rot(api, oracle):
    """the rotation's arrays on the device (r) beside the host's (d), the accepted rows alone per size, and a blinding context"""
    import torch
    d = sc.rotation_set(oracle)
    r = {k: up(a.view(np.int32) if a.dtype == np.uint32 else a) for k, a in d.items()
         if isinstance(a, np.ndarray) and a.ndim == 2 and a.dtype in (np.uint8, np.uint32)}
    r["offsets"] = up(sc.ragged_offsets(sc.ROT_LARGE, sc.ROT_MSG_LEN).view(np.int64))
    valid = {}
    for m in (sc.ROT_SMALL, sc.ROT_LARGE):
        rows = d["valid_rows"][d["valid_rows"] < m]
        valid[m] = {k: up(d[k][rows].view(np.int32) if d[k].dtype == np.uint32 else d[k][rows]) for k in ("v_sig", "v_pk", "v_msg", "v_idx")}
    L = _lib.load()
    bctx = np.zeros(192, np.uint8)
    seed = np.frombuffer(b"streams", np.uint8).copy()
    assert L.ed25519_Blinding_Init(bctx.ctypes.data, seed.ctypes.data, len(seed)) == bctx.ctypes.data
    r["bctx"] = up(bctx.reshape(1, 192))
    torch.cuda.synchronize()
    return d, r, valid


# ---- jobs: (enqueue on the current stream, compare afterwards, the hook that reports the call's path, the stream's number) ------
def verify_job(api, one_key, rules, name, stream):
    key, n = sc.VERIFY_CALLS[name]
    k = one_key[key]
    out = verdicts(n)

    def enqueue():
        api.ed25519_Verify_Check_dev(out, k["ctx"], k["sig"][:n], k["msg"][:n], rules)

    def compare():
        got = host(out).reshape(n)
        assert np.array_equal(got, k["ok"][:n]), ("Verify_Check", rules, name, int((got != k["ok"][:n]).sum()))

    return enqueue, compare, check_hook, stream


def peer_job(api, one_peer, name, stream):
    peer, n = sc.PEER_CALLS[name]
    p = one_peer[peer]
    sk = one_peer["sk"][:n].clone()                        # (the call clamps it in place)
    out = filled(n, 32)

    def enqueue():
        api.curve25519_dh_CreateSharedKey_one_peer_dev(out, p["pk"], sk)

    def compare():
        got = host(out)
        want = sc.tile(p["shared"], n)
        assert np.array_equal(got, want), ("one_peer", name, int((got != want).any(axis=1).sum()))
        assert np.array_equal(host(sk), sc.tile(p["clamped"], n)), ("one_peer secrets", name)
        if peer == "minus_one":
            assert not got.any()

    return enqueue, compare, peer_hook, stream


def run(jobs, streams, hooks):
    """every job enqueued on its stream, in order; ONE synchronise; then every comparison.  hooks: read each job's hook behind its
    call (which synchronises with that call's stream).  Returns what the hooks said."""
    import torch
    torch.cuda.synchronize()                               # uploads, fills and clones are done: from here on nothing but the calls
    said = []
    for enqueue, _, hook, s in jobs:
        with torch.cuda.stream(streams[s]):
            enqueue()
        if hooks:
            said.append(hook())
    torch.cuda.synchronize()
    for _, compare, _, _ in jobs:
        compare()
    return said


def zip215_walks_every_size(rules):
    """the ZIP-215 form hands a call below ZIP215_CHECK_MIN (2^16) to the per-element kernels, which keep nothing: with the tunable
    at 0 its small calls ask the kept buffer like the other two forms'"""
    return _lib.tunable("ZIP215_CHECK_MIN", 0) if rules == "zip215" else contextlib.nullcontext()


# ---- a ------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("order", list(sc.VERIFY_ORDERS))
@pytest.mark.parametrize("rules", ("plain", "strict", "zip215"))
def test_key_comb_handed_over_in_flight(api, streams, one_key, one_peer, rules, order, hooks):
    """A (2^17 pairs under K0) builds and walks K0's comb on one stream while B (2^16 under K1), enqueued at once on another,
    rebuilds the kept buffer; C (4096 under K0) finds another key remembered and D (4096 under K1) its own: the oracle's verdicts
    for all four, in every order of the two streams and on one stream"""
    fresh_thread_state(api, streams, one_peer)
    jobs = [verify_job(api, one_key, rules, name, s) for name, s in sc.VERIFY_ORDERS[order]]
    with zip215_walks_every_size(rules):
        said = run(jobs, streams, hooks)
    if hooks:
        assert said == sc.check_paths([sc.VERIFY_CALLS[name] for name, _ in sc.VERIFY_ORDERS[order]]), (rules, order)


# ---- b ------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("order", list(sc.PEER_ORDERS))
def test_peer_comb_handed_over_in_flight(api, streams, one_peer, order, hooks):
    """the same for curve25519_dh_CreateSharedKey_one_peer_dev: A (2^19 secrets: the comb is walked at 1.3 G/s, so 2^17 are gone in
    0.1 ms, before the next call's kernels can reach the device) walks p0's comb while B rebuilds it for p1; a twist peer and
    u = p - 1 are refused on the device (the ladder decides them, the last refused key is written into the same kept buffer);
    then p0 finds p1 remembered and p1 its own comb.  The orders: tests/stream_cases.py, above PEER_ORDERS"""
    fresh_thread_state(api, streams, one_peer)
    jobs = [peer_job(api, one_peer, name, s) for name, s in sc.PEER_ORDERS[order]]
    said = run(jobs, streams, hooks)
    if hooks:
        assert said == sc.peer_paths([sc.PEER_CALLS[name] for name, _ in sc.PEER_ORDERS[order]]), order


# ---- c ------------------------------------------------------------------------------------------------------------------------
@MODES
def test_both_kept_buffers_at_once(api, streams, one_key, one_peer, hooks):
    """a's and b's calls in turn over three streams: the two kept buffers are ordered each for itself, a verification neither
    waits for nor tramples the peer's comb"""
    fresh_thread_state(api, streams, one_peer)
    jobs = [verify_job(api, one_key, "plain", name, s) if kind == "verify" else peer_job(api, one_peer, name, s)
            for kind, name, s in sc.BOTH_ORDER]
    said = run(jobs, streams, hooks)
    if hooks:
        want_v = sc.check_paths([sc.VERIFY_CALLS[name] for kind, name, _ in sc.BOTH_ORDER if kind == "verify"])
        want_p = sc.peer_paths([sc.PEER_CALLS[name] for kind, name, _ in sc.BOTH_ORDER if kind == "peer"])
        assert [v for v, (kind, _, _) in zip(said, sc.BOTH_ORDER) if kind == "verify"] == want_v
        assert [v for v, (kind, _, _) in zip(said, sc.BOTH_ORDER) if kind == "peer"] == want_p


# ---- d: every other call ------------------------------------------------------------------------------------------------------
# A chain enqueues its calls on the current stream for the first m rows and returns [(label, device tensor, expected array)]: where
# one call's output is the next one's input (Init, then the indexed call) both are in one chain, so on one stream.
def chains(api, d, r, valid):
    from curve25519_amd.api import PEER_CTX_SIZE, SIGN_CTX_SIZE
    L = _lib.load()
    K, W = sc.ROT_KEYS, sc.ROT_MSG_LEN

    def ok(rc, what):
        _lib.check(rc, what)

    def peer_indexed(m):
        ctx, sk, out = filled(K, PEER_CTX_SIZE), r["xsk"][:m].clone(), filled(m, 32)
        api.curve25519_dh_Peer_Init_dev(ctx, r["xpk"])
        api.curve25519_dh_CreateSharedKey_indexed_dev(out, ctx, r["idx"][:m], sk)
        return [("shared", out, d["shared"][:m]), ("clamped secrets", sk, d["xsk_clamped"][:m])]

    def sign_indexed(m):
        ctx, sig = filled(K, SIGN_CTX_SIZE), filled(m, 64)
        api.ed25519_Sign_Init_dev(ctx, r["priv"])
        api.ed25519_SignMessage_indexed_dev(sig, ctx, r["idx"][:m], r["msg"][:m])
        return [("signatures", sig, d["sig"][:m])]

    def sign_indexed_ragged(m):
        ctx, sig = filled(K, SIGN_CTX_SIZE), filled(m, 64)
        api.ed25519_Sign_Init_dev(ctx, r["priv"])
        ok(L.ed25519_SignMessage_indexed_ragged_dev(ptr(sig), ptr(ctx), K, ptr(r["idx"]), ptr(r["msg"]), ptr(r["offsets"]), m, cur()),
           "ed25519_SignMessage_indexed_ragged_dev")
        return [("signatures", sig, d["sig"][:m])]

    def verify_init():
        ctx = filled(K, 2080)
        ok(L.ed25519_Verify_Init_dev(ptr(ctx), ptr(r["pub"]), K, cur()), "ed25519_Verify_Init_dev")
        return ctx

    def check_indexed(zip215):
        def chain(m):
            ctx, out = verify_init(), verdicts(m)
            api.ed25519_Verify_Check_indexed_dev(out, ctx, r["v_idx"][:m], r["v_sig"][:m], r["v_msg"][:m], zip215=zip215)
            return [("verdicts", out, d["v_ok"][:m])]
        return chain

    def check_indexed_ragged(name):
        def chain(m):
            ctx, out = verify_init(), verdicts(m)
            ok(getattr(L, name)(ptr(out), ptr(ctx), K, ptr(r["v_idx"]), ptr(r["v_sig"]), ptr(r["v_msg"]), ptr(r["offsets"]), m, cur()), name)
            return [("verdicts", out, d["v_ok"][:m])]
        return chain

    def verify(fn, pk, want):
        def chain(m):
            out = verdicts(m)
            fn(out, r["v_sig"][:m], r[pk][:m], r["v_msg"][:m])
            return [("verdicts", out, d[want][:m])]
        return chain

    def verify_ragged(name, pk, want):
        def chain(m):
            out = verdicts(m)
            ok(getattr(L, name)(ptr(out), ptr(r["v_sig"]), ptr(r[pk]), ptr(r["v_msg"]), ptr(r["offsets"]), m, cur()), name)
            return [("verdicts", out, d[want][:m])]
        return chain

    def batch(m):
        v, yes, no = valid[m], verdicts(1), verdicts(1)
        api.ed25519_VerifyBatch_zip215_dev(yes, v["v_sig"], v["v_pk"], v["v_msg"], SEED)
        api.ed25519_VerifyBatch_zip215_dev(no, r["v_sig"][:m], r["v_pk"][:m], r["v_msg"][:m], SEED)
        return [("accepted rows alone", yes, np.ones((1, 1), np.int32)), ("all rows", no, np.zeros((1, 1), np.int32))]

    def batch_indexed(m):
        v, yes, no = valid[m], verdicts(1), verdicts(1)
        api.ed25519_VerifyBatch_zip215_indexed_dev(yes, r["pub"], v["v_idx"], v["v_sig"], v["v_msg"], SEED)
        api.ed25519_VerifyBatch_zip215_indexed_dev(no, r["pub"], r["v_idx"][:m], r["v_sig"][:m], r["v_msg"][:m], SEED)
        return [("accepted rows alone", yes, np.ones((1, 1), np.int32)), ("all rows", no, np.zeros((1, 1), np.int32))]

    def keys(m):
        flags, xpk, good, xsk = verdicts(m), filled(m, 32), verdicts(m), filled(m, 32)
        api.ed25519_ClassifyKey_dev(flags, r["c_keys"][:m])
        api.ed25519_PublicKey_to_X25519_dev(xpk, good, r["c_keys"][:m])
        api.ed25519_PrivateKey_to_X25519_dev(xsk, r["priv_rows"][:m])
        return [("flags", flags, d["c_flags"][:m].view(np.int32)), ("converted keys", xpk, d["c_xpk"][:m]), ("ok", good, d["c_ok"][:m]),
                ("converted secrets", xsk, d["c_xsk"][:m])]

    def key_pairs(m):
        pub, priv, pk, fast, sk1, sk2 = filled(m, 32), filled(m, 64), filled(m, 32), filled(m, 32), r["xsk"][:m].clone(), r["xsk"][:m].clone()
        api.ed25519_CreateKeyPair_dev(pub, priv, r["xsk"][:m])
        api.curve25519_dh_CalculatePublicKey_dev(pk, sk1)
        api.curve25519_dh_CalculatePublicKey_dev(fast, sk2, fast=True)
        return [("public keys", pub, d["kp_pub"][:m]), ("private keys", priv, d["kp_priv"][:m]), ("X25519 public keys", pk, d["x_pub"][:m]),
                ("X25519 public keys, fast", fast, d["x_pub_fast"][:m]), ("clamped", sk1, d["xsk_clamped"][:m]), ("clamped, fast", sk2, d["xsk_clamped"][:m])]

    def blinded(m):
        pub, priv, sig = filled(m, 32), filled(m, 64), filled(m, 64)
        ok(L.ed25519_CreateKeyPair_blinded_dev(ptr(pub), ptr(priv), ptr(r["bctx"]), ptr(r["xsk"]), m, cur()), "ed25519_CreateKeyPair_blinded_dev")
        ok(L.ed25519_SignMessage_blinded_dev(ptr(sig), ptr(r["priv_rows"]), ptr(r["bctx"]), ptr(r["msg"]), W, m, cur()), "ed25519_SignMessage_blinded_dev")
        return [("public keys", pub, d["kp_pub"][:m]), ("private keys", priv, d["kp_priv"][:m]), ("signatures", sig, d["sig"][:m])]

    return {
        "peer_indexed": peer_indexed, "sign_indexed": sign_indexed, "sign_indexed_ragged": sign_indexed_ragged,
        "check_indexed": check_indexed(False), "check_zip215_indexed": check_indexed(True),
        "check_indexed_ragged": check_indexed_ragged("ed25519_Verify_Check_indexed_ragged_dev"),
        "check_zip215_indexed_ragged": check_indexed_ragged("ed25519_Verify_Check_zip215_indexed_ragged_dev"),
        "verify": verify(api.ed25519_VerifySignature_dev, "g_pk", "g_ok"),
        "verify_strict": verify(api.ed25519_VerifySignature_strict_dev, "v_pk", "v_ok"),
        "verify_zip215": verify(api.ed25519_VerifySignature_zip215_dev, "g_pk", "g_ok"),
        "verify_strict_ragged": verify_ragged("ed25519_VerifySignature_strict_ragged_dev", "v_pk", "v_ok"),
        "verify_zip215_ragged": verify_ragged("ed25519_VerifySignature_zip215_ragged_dev", "g_pk", "g_ok"),
        "batch": batch, "batch_indexed": batch_indexed, "keys": keys, "key_pairs": key_pairs, "blinded": blinded,
    }


def compare_all(results):
    for name, m, label, out, want in results:
        got = host(out).reshape(want.shape)
        assert np.array_equal(got, want), (name, m, label, int((got != want).sum()))


def test_every_other_call_in_a_six_stream_rotation(api, streams, rot):
    """seventeen chains of calls, three rounds, six streams, two sizes per chain (four lanes per element, and one): the four work
    slabs are shared, regrown and handed from stream to stream while kernels run, each slab with a slow list of its own where the
    plain and the ZIP-215 verification meet a garbage key; the batch equations run at these sizes (BATCH_EQ_MIN and
    BATCH_EQ_INDEXED_MIN at 1).  One synchronise at the end, every result the oracle's or the model's"""
    import torch
    d, r, valid = rot
    release()
    table = chains(api, d, r, valid)
    results = []
    torch.cuda.synchronize()
    with _lib.tunable("BATCH_EQ_MIN", 1), _lib.tunable("BATCH_EQ_INDEXED_MIN", 1):
        for rnd in range(3):
            for j, (name, chain) in enumerate(table.items()):
                m = sc.ROT_LARGE if (j + rnd) & 1 else sc.ROT_SMALL
                with torch.cuda.stream(streams[(j + rnd) % len(streams)]):
                    results += [(name, m, label, out, want) for label, out, want in chain(m)]
    torch.cuda.synchronize()
    compare_all(results)


# ---- e: the three last-call hooks ---------------------------------------------------------------------------------------------
def test_hooks_report_the_last_call_of_their_kind(api, streams, one_key, one_peer, rot):
    """After an interleaved run and WITHOUT a synchronise, each hook reports the thread's last call of its kind: not an older one
    (whose answer was the opposite), and not whatever later calls of other kinds on the same stream left in the slab.  Twice, with
    the answers the other way round; -1 from all three once the thread's state is released"""
    import torch
    d, r, valid = rot
    release()
    assert (check_hook(), peer_hook(), slow_hook()) == (-1, -1, -1)
    table = chains(api, d, r, valid)
    big, small = sc.ROT_LARGE, sc.ROT_SMALL
    slow = sc.slow_rows(d, big)
    assert slow > 0
    results, jobs = [], []

    def chain(name, m, s):
        with torch.cuda.stream(streams[s]):
            results.extend((name, m, label, out, want) for label, out, want in table[name](m))

    def job(j):
        enqueue, compare, _, s = j
        jobs.append(j)
        with torch.cuda.stream(streams[s]):
            enqueue()

    def verify_clean(m, s):                                 # the plain call on keys that all decode: an empty slow list
        with torch.cuda.stream(streams[s]):
            out = verdicts(m)
            api.ed25519_VerifySignature_dev(out, r["v_sig"][:m], r["v_pk"][:m], r["v_msg"][:m])
            results.append(("verify, clean keys", m, "verdicts", out, d["v_ok"][:m]))

    torch.cuda.synchronize()
    # older calls: the combs are built and walked (1, 1), garbage keys are listed
    job(verify_job(api, one_key, "plain", "B", 0))
    job(peer_job(api, one_peer, "B", 1))
    chain("verify", big, 2)
    chain("sign_indexed", small, 3)
    # the last call of each kind: another key than the remembered one (0), another peer (0), no key that fails to decode (0) ...
    job(verify_job(api, one_key, "plain", "C", 1))
    job(peer_job(api, one_peer, "C", 2))
    verify_clean(big, 1)                                    # (its per-element tables cover the whole slab of the call before it)
    # ... and behind each, on its stream, calls of other kinds that use the same slab
    chain("sign_indexed", big, 1)
    chain("key_pairs", big, 2)
    chain("keys", big, 0)
    chain("blinded", big, 4)
    chain("peer_indexed", big, 5)
    assert (check_hook(), peer_hook(), slow_hook()) == (0, 0, 0)
    # the other way round
    job(verify_job(api, one_key, "plain", "D", 2))
    job(peer_job(api, one_peer, "D", 0))
    chain("verify", big, 1)
    chain("sign_indexed", big, 2)
    chain("key_pairs", big, 0)
    chain("keys", big, 1)
    chain("sign_indexed_ragged", small, 5)
    assert (check_hook(), peer_hook(), slow_hook()) == (1, 1, slow)
    torch.cuda.synchronize()
    for _, compare, _, _ in jobs:
        compare()
    compare_all(results)
    release()
    assert (check_hook(), peer_hook(), slow_hook()) == (-1, -1, -1)
