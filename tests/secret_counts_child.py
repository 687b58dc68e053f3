"""The profiled child of tests/test_gpu_secret_counts.py (run under `rocprofv3 --pmc ... -- python tests/secret_counts_child.py
<out dir>`): every secret-bearing *_dev call at one size inside each of its default dispatch ranges, once per SECRET CLASS with
identical public inputs, a marker kernel between the calls; then the two probe kernels of tests/ct_probe.hip on all-zero and
all-ones input.  Writes <out dir>/manifest.json: the list of segments in dispatch order, one per marker.

Classes 0-3 are uniform across the call (every row the same secret), so that a secret-dependent branch would be wave-uniform and
skip instructions; class 4 has independent random rows; class 5 repeats class 2 (the control).  Every call gets fresh copies of its
secrets (the calls clamp in place), after one warm-up call per kind and size that builds the kept state (combs, scratch)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

MSG_LEN = 80
N_CTX = 5
CLASSES = ("zeros", "ones", "uniform_a", "uniform_b", "random_rows", "uniform_a_again")
# 1, then the first size of each default dispatch range (tests/dispatch_cases.py; the thresholds of the other calls are pinned by
# their own GPU tests: ONE_PEER_WIDE = 3 << 15, PEER_INDEXED_MIN = 2049, the blinded calls' 2048)
SIZES = {
    "x25519": (1, 513, 3585, 32769),
    "x25519_one_peer": (1, 4097, (3 << 15) + 1),
    "x25519_indexed": (1, 2049, 3585),
    "public_key": (1, 513, 3585, 32769),
    "public_key_fast": (1, 513, 3585, 32769),
    "keypair": (1, 1025, 16385),
    "sign": (1, 1025, 16385),
    "keypair_blinded": (1, 2049),
    "sign_blinded": (1, 2049),
    "sign_indexed": (1, 1025, 16385),
    "private_to_x25519": (1, 1025),
}
PROBE_N = 4096


def secret_rows(cls: int, n: int, width: int, seed: int) -> np.ndarray:
    """uint8[n, width] of secret class `cls`"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, width, np.uint8), rng.integers(0, 256, width, np.uint8)
    if cls == 0:
        return np.zeros((n, width), np.uint8)
    if cls == 1:
        return np.full((n, width), 0xFF, np.uint8)
    if cls in (2, 5):
        return np.tile(a, (n, 1))
    if cls == 3:
        return np.tile(b, (n, 1))
    return np.random.default_rng(seed + 1).integers(0, 256, (n, width), np.uint8)


def main(out_dir):
    probe_so = os.path.join(out_dir, "libct_probe.so")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", os.path.join(HERE, "ct_probe.hip"), "-o", probe_so])
    import torch
    from curve25519_amd import _lib, api
    L = _lib.load()
    dev = torch.device("cuda", 0)
    probe = C.CDLL(probe_so)
    probe.ct_probe_launch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    probe.ct_marker_launch.argtypes = [C.c_void_p, C.c_void_p]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def empty(n, w):
        return torch.empty((n, w), dtype=torch.uint8, device=dev)

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    marker_count = torch.zeros(1, dtype=torch.int32, device=dev)
    manifest = []

    def segment(**what):
        """everything dispatched from here to the next segment() belongs to `what`"""
        torch.cuda.synchronize()
        assert probe.ct_marker_launch(P(marker_count), stream()) == 0
        torch.cuda.synchronize()
        manifest.append(what)

    pub = lambda n, w, seed: np.random.default_rng(seed).integers(0, 256, (n, w), np.uint8)  # noqa: E731

    # public state shared by the classes of a kind: one eligible peer key, peer contexts, the message, the index
    one_peer_pk = None
    for seed in range(64):
        cand = pub(1, 32, 9000 + seed)
        ctx = api.curve25519_dh_Peer_Init(cand)
        if int(np.frombuffer(ctx[0, 32:36].tobytes(), np.uint32)[0]) == 1:      # the context's eligibility word
            one_peer_pk = cand
            break
    assert one_peer_pk is not None
    peer_keys = np.concatenate([one_peer_pk, pub(N_CTX - 1, 32, 9100)])
    peer_ctxs = up(api.curve25519_dh_Peer_Init(peer_keys))

    def call(kind, n, secret, blind):
        """one *_dev call of `kind` on n rows; secret: uint8[n, 32] (uint8[N_CTX, 128] for sign_indexed), blind: uint8[1, 192]"""
        idx = up((np.arange(n, dtype=np.int32) % N_CTX).reshape(n, 1))
        msg = up(pub(n, MSG_LEN, 9200))
        if kind != "sign_indexed":
            priv = np.concatenate([secret, pub(n, 32, 9300)], axis=1)            # seed || a public half, the same in every class
        if kind == "x25519":
            api.curve25519_dh_CreateSharedKey_dev(empty(n, 32), up(pub(n, 32, 9400)), up(secret))
        elif kind == "x25519_one_peer":
            api.curve25519_dh_CreateSharedKey_one_peer_dev(empty(n, 32), up(one_peer_pk), up(secret))
        elif kind == "x25519_indexed":
            api.curve25519_dh_CreateSharedKey_indexed_dev(empty(n, 32), peer_ctxs, idx, up(secret))
        elif kind == "public_key":
            api.curve25519_dh_CalculatePublicKey_dev(empty(n, 32), up(secret))
        elif kind == "public_key_fast":
            api.curve25519_dh_CalculatePublicKey_dev(empty(n, 32), up(secret), fast=True)
        elif kind == "keypair":
            api.ed25519_CreateKeyPair_dev(empty(n, 32), empty(n, 64), up(secret))
        elif kind == "sign":
            api.ed25519_SignMessage_dev(empty(n, 64), up(priv), msg)
        elif kind == "keypair_blinded":
            pub_out, priv_out, b, sk = empty(n, 32), empty(n, 64), up(blind), up(secret)
            _lib.check(L.ed25519_CreateKeyPair_blinded_dev(P(pub_out), P(priv_out), P(b), P(sk), n, stream()), kind)
        elif kind == "sign_blinded":
            sig, b, pr = empty(n, 64), up(blind), up(priv)
            _lib.check(L.ed25519_SignMessage_blinded_dev(P(sig), P(pr), P(b), P(msg), MSG_LEN, n, stream()), kind)
        elif kind == "sign_indexed":
            api.ed25519_SignMessage_indexed_dev(empty(n, 64), up(secret), idx, msg)
        elif kind == "private_to_x25519":
            api.ed25519_PrivateKey_to_X25519_dev(empty(n, 32), up(priv))
        else:
            raise AssertionError(kind)
        torch.cuda.synchronize()

    def inputs(kind, n, cls):
        """(secret, blinding context) of one class: the contexts of sign_indexed are secret in all their 128 bytes"""
        if kind == "sign_indexed":
            return secret_rows(cls, N_CTX, 128, 77), None
        return secret_rows(cls, n, 32, 77), secret_rows(cls, 1, 192, 78)

    for kind, sizes in SIZES.items():
        for n in sizes:
            segment(kind=kind, n=n, cls="warmup")
            call(kind, n, *inputs(kind, n, 4))
            for cls in range(len(CLASSES)):
                secret, blind = inputs(kind, n, cls)
                segment(kind=kind, n=n, cls=CLASSES[cls])
                call(kind, n, secret, blind)

    # the proof that the method sees a leak
    out = torch.empty(PROBE_N, dtype=torch.int32, device=dev)
    for select in (0, 1):
        for name, value in (("zeros", 0), ("ones", -1)):
            secret = torch.full((PROBE_N,), value, dtype=torch.int32, device=dev)
            segment(kind="probe_select" if select else "probe_branch", n=PROBE_N, cls=name)
            assert probe.ct_probe_launch(select, P(out), P(secret), PROBE_N, stream()) == 0
            torch.cuda.synchronize()
    segment(kind="end", n=0, cls="end")
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f)


if __name__ == "__main__":
    main(sys.argv[1])
