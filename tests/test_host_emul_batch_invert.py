"""CPU tests of the shared inversion's device source (curve25519_amd/csrc/batch_invert.cuh: the body of k_batch_invert, the last
kernel of every large batch).  The same source is compiled by g++ and run as waves of 64 lock-step lanes (tests/host_emul/coop_wave.h:
the quads' quad_perm exchange as rendezvous), at every instantiated group size and at ragged sizes, with zeros placed on the slot
map (tests/invert_cases.py) in every limb form the producers store.  Every 1 / z must equal z^(p-2) mod p, and 0 where z = 0."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import invert_cases as cases


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_batch_invert": ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int)})
    yield lib
    assert_no_mad_overflow(lib)


def invert(lib, limbs, n, k):
    out = np.full((n, 8), 0xA5A5A5A5, np.uint32)           # (an element the model never writes cannot pass as 0)
    got_k = lib.emul_batch_invert(out.ctypes.data, np.ascontiguousarray(limbs).ctypes.data, n, k)
    assert got_k == cases.group(k)
    return out


@pytest.mark.parametrize("K", cases.INSTANTIATED)
def test_every_group_size_against_big_integers(lib, K):
    """ragged sizes (lanes m = ceil(n / K) not a multiple of the quad or the wave, the last slot live on some lanes only), zeros
    on every slot, a whole lane, a whole quad, the last slot only, the last live lane and a sprinkle -- as limbs of 0, of p and
    inflated to the bound -- between edge vectors of the stored class"""
    for n in cases.hook_sizes(K):
        slots = cases.batch_slots(n, K)
        pats = cases.zero_patterns(slots, seed=n)
        zeros = cases.all_zeros(pats)
        limbs, vals = cases.make_inputs(n, zeros, seed=n + K)
        got = invert(lib, limbs, n, K)
        want = cases.expected(vals)
        bad, count = cases.mismatches(got, want, vals, pats)
        assert count == 0, f"K={K} n={n}: {count} wrong, {bad}"
        if n > 64 * K:
            for name in ("lane_all_zero", "quad_all_zero", "every_slot", "last_live_lane"):
                assert name in pats, f"K={K} n={n}: no room for {name}"
            if K > 1:
                assert "last_slot_only" in pats


def test_requested_sizes_round_down(lib):
    """what the hook and INV_K accept rounds down to an instantiated size: 3 -> 2, 13 -> 12, 15 -> 14, above 16 -> 16"""
    n = cases.ragged_n(67, 12, 5)
    slots = cases.batch_slots(n, 12)
    zeros = cases.all_zeros(cases.zero_patterns(slots, seed=3))
    limbs, vals = cases.make_inputs(n, zeros, seed=4)
    want = cases.expected(vals)
    for k in (3, 13, 15, 17):
        got = invert(lib, limbs, n, k)
        assert (got == want).all(), k


def test_no_zero_and_all_zero(lib):
    """a batch without a zero (every quad inverts a product of K*4 real factors) and a batch of nothing but zeros (every quad
    inverts 1)"""
    for K in (1, 8, 16):
        n = cases.ragged_n(69, K, 1)
        limbs, vals = cases.make_inputs(n, set(), seed=K)
        assert (invert(lib, limbs, n, K) == cases.expected(vals)).all(), K
        limbs, vals = cases.make_inputs(n, set(range(n)), seed=K)
        assert not invert(lib, limbs, n, K).any(), K


def test_slot_maps_cover_every_element():
    """the generator's maps themselves: every element once, k_batch_invert's lanes in whole waves, the fused kernel's in whole
    workgroups"""
    for n in (1, 63, 65, 1000, 4097):
        for K in cases.INSTANTIATED:
            s = cases.batch_slots(n, K)
            assert sorted(s[s >= 0].tolist()) == list(range(n)) and s.shape[0] % 64 == 0
        for block in (64, 128, 256, 512):
            s = cases.fused_slots(n, block)
            assert sorted(s[s >= 0].tolist()) == list(range(n)) and s.shape[1] == block // 64
