"""Inputs for the shared inversion (curve25519_amd/csrc/batch_invert.cuh, k_batch_invert; k_x25519_fused's inverting wave) and
their big-integer answer.  Montgomery's trick goes wrong along its slot map: which element a lane holds in which slot, what a lane
past the end multiplies in, and where a zero is swapped for one.  So the cases are built from the map itself -- for n elements at
K per lane, lane j of k_batch_invert holds e = j + t*m (m = ceil(n / K)), lane tid of a k_x25519_fused workgroup e = blk*64K +
tid + 64t -- and the zeros are placed on it: every slot of a lane, a whole quad, only the last slot, the last live lane beside
partners past the end, and a sparse sprinkle.  Shared by the CPU model's test (tests/test_host_emul_batch_invert.py) and the
device's (tests/test_gpu_batch_invert.py)."""
import random

import numpy as np

import limb_vectors as lv

P = 2**255 - 19
INSTANTIATED = (1, 2, 4, 8, 12, 14, 16)       # the group sizes k_batch_invert is instantiated for
HOOK_K = (1, 2, 3, 4, 8, 12, 13, 14, 15, 16, 0)   # what the self-test hook is asked for (0: its built-in choice)
QUAD = 4
WAVE = 64


def group(k: int) -> int:
    """k elements per lane rounded down to an instantiated size (batch_invert.cuh: inversion_group)."""
    return max(g for g in INSTANTIATED if g <= max(k, 1))


def batch_slots(n: int, K: int) -> np.ndarray:
    """k_batch_invert's map: [lanes, K] element indices (-1 past the end), lanes = m rounded up to whole waves."""
    m = -(-n // K)
    lanes = -(-m // WAVE) * WAVE
    j = np.arange(lanes)[:, None]
    e = j + np.arange(K)[None, :] * m
    return np.where((j < m) & (e < n), e, -1)


def fused_slots(n: int, block: int) -> np.ndarray:
    """k_x25519_fused's map: [workgroups * 64, K] element indices (-1 past the end), K = block / 64; row blk*64 + tid is the
    inverting lane tid of workgroup blk."""
    K = block // WAVE
    blocks = -(-n // block)
    b = np.arange(blocks)[:, None, None]
    tid = np.arange(WAVE)[None, :, None]
    t = np.arange(K)[None, None, :]
    e = (b * block + tid + WAVE * t).reshape(blocks * WAVE, K)
    return np.where(e < n, e, -1)


def ragged_n(m: int, K: int, r: int) -> int:
    """the n with ceil(n / K) = m whose last slot is live on r of K ... m - K + r lanes (1 <= r <= K)"""
    return K * (m - 1) + r


def zero_patterns(slots: np.ndarray, seed: int = 0) -> dict:
    """Where the zeros go on a slot map: name -> sorted element indices.  Each pattern sits on lanes of its own (quads apart
    where the map is wide enough), so one input can carry all of them."""
    rng = random.Random(seed)
    lanes, K = slots.shape
    live = [j for j in range(lanes) if slots[j, 0] >= 0]
    full = [j for j in live if (slots[j] >= 0).all()]
    used = set()

    def take(cands):
        for j in cands:
            if j // QUAD not in used:
                used.add(j // QUAD)
                return j
        return None

    out = {}
    last = live[-1]
    used.add(last // QUAD)
    out["last_live_lane"] = [int(e) for e in slots[last] if e >= 0]   # partners past the end where the lanes do not fill the quad
    j = take(full[len(full) // 2:] + full)
    if j is not None:
        out["lane_all_zero"] = [int(e) for e in slots[j]]
    quads = [q for q in range(lanes // QUAD) if all((slots[QUAD * q + i] >= 0).all() for i in range(QUAD)) and q not in used]
    if quads:
        q = quads[len(quads) // 3]
        used.add(q)
        out["quad_all_zero"] = [int(e) for i in range(QUAD) for e in slots[QUAD * q + i]]
    j = take(full[len(full) // 4:] + full)
    if j is not None and K > 1:
        out["last_slot_only"] = [int(slots[j, K - 1])]
    picks = []
    for t in range(K):                                  # every slot t, each on another lane
        cand = [j for j in live if slots[j, t] >= 0 and j // QUAD not in used]
        if cand:
            j = cand[rng.randrange(len(cand))]
            used.add(j // QUAD)
            picks.append(int(slots[j, t]))
    out["every_slot"] = picks
    n_live = int((slots >= 0).sum())
    free = [int(e) for j in live if j // QUAD not in used for e in slots[j] if e >= 0]
    out["sprinkle"] = sorted(rng.sample(free, min(len(free), max(1, n_live // 97)))) if free else []
    return {k: sorted(v) for k, v in out.items() if v}


def all_zeros(patterns: dict) -> set:
    return set(e for v in patterns.values() for e in v)


def value_pool(seed: int = 0):
    """(nonzero limb vectors, zero limb vectors) of the class the producers store in the scratch (tools/fe_bounds.py's reduced
    class: the output of a carry chain): random canonical values, 1, p - 1, the class's edge vectors (tests/limb_vectors.py);
    zero as the limbs of 0, of p, and inflated to the bound."""
    rng = random.Random(seed)
    nonzero, zero = [], [list(lv.ZERO), lv.canonical_limbs(P)]
    for v in (1, P - 1, 2, 19, P - 19):
        nonzero.append(lv.canonical_limbs(v))
    for vec in lv.classes(lv.R, rng):
        (zero if lv.value(vec) % P == 0 else nonzero).append(vec)
    return nonzero, zero


def make_inputs(n: int, zeros, seed: int = 0):
    """n field elements in the scratch's SoA layout (limb w of element e at w*n + e), uint32[10 * n], and their values: element e
    is zero (mod p) iff e in `zeros`.  The edge vectors and random canonical values alternate."""
    rng = random.Random(seed)
    nonzero, zero = value_pool(seed)
    limbs = np.zeros((10, n), np.uint32)
    vals = []
    zi = 0
    for e in range(n):
        if e in zeros:
            vec = zero[zi % len(zero)]
            zi += 1
        elif e % 3 == 0:
            vec = nonzero[(e // 3) % len(nonzero)]
        else:
            vec = lv.canonical_limbs(rng.randrange(1, P))
        limbs[:, e] = vec
        vals.append(lv.value(vec) % P)
    return limbs.reshape(-1), vals


def expected(vals) -> np.ndarray:
    """uint32[n, 8]: the canonical words of z^(p-2) mod p (0 for z = 0), what the reference's ecp_Inverse gives."""
    out = np.zeros((len(vals), 8), np.uint32)
    for e, v in enumerate(vals):
        r = pow(v, P - 2, P)
        out[e] = [(r >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    return out


def hook_sizes(K: int):
    """ragged sizes for group size K: m = ceil(n / K) lanes with m mod 4 in {1, 2, 3}, m mod 64 != 0, up to a few waves of quads,
    the last slot live on some lanes only"""
    out = [1, 2, 5]
    for m, r in ((3, 1), (7, K), (66, max(1, K - 1)), (64 * 4 + 3, max(1, K // 2)), (64 * 4 * 2 + 5, 1)):
        out.append(ragged_n(m, K, r))
    return sorted(set(out))


def mismatches(got: np.ndarray, want: np.ndarray, vals, patterns=None):
    """the first few wrong elements, described"""
    bad = np.nonzero((got != want).any(axis=1))[0]
    where = {e: k for k, v in (patterns or {}).items() for e in v}
    return [f"e={e} z={hex(vals[e])} zero_pattern={where.get(int(e))}" for e in bad[:6]], len(bad)
