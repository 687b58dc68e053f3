// curve25519_amd/csrc/batch_invert_lane.inc -- the work of ONE lane of the shared inversion, included as the body of k_batch_invert
// (engine_common.cuh) and of its CPU model (tests/host_emul/emul.cpp: emul_batch_invert), so that both run the same source.
// It is a fragment rather than a function because the product kernels' ISA must not change: the same statements as a C25519_DEV
// function inlined into the kernel compile to different (equivalent) instructions.
//
// In scope where it is included: template parameters Fin, K; Z (the scratch's SoA Z's), n, m (lanes = ceil(n / K)), fin (Fin::emit),
// pre_lds ((K-1) x 10 x INV_BLOCK words of LDS, used at K > 14), blockIdx, threadIdx.  Lane j = blockIdx.x * INV_BLOCK + threadIdx.x
// owns elements j, j + m, ..., j + (K-1) m: prefix products forward, ONE inversion per quad of lanes, unwinding backwards; a zero Z
// takes no part and gets 0.  Every lane of the wave must get here: the quad's exchange needs its partners, live or not.
    constexpr bool PREFIX_IN_LDS = K > 14;
    const size_t j = (size_t)blockIdx.x * INV_BLOCK + threadIdx.x;
    const bool live = j < m;                                // (a lane past the end stays: its quad shares the inversion below)
    fe z[K], pre[PREFIX_IN_LDS ? 1 : K];
    u32 zero_mask = 0;
#pragma unroll
    for (int t = 0; t < K; t++) {
        const size_t e = j + (size_t)t * m;
        if (live && e < n) soa_load_fe(z[t], Z, n, e);
        else fe_set_u32(z[t], 1);                           // past the end: a factor of one
    }
    fe acc;
#pragma unroll
    for (int t = 0; t < K; t++) {
        zero_mask |= (fe_zero_to_one(z[t]) & 1u) << t;      // z == 0 (mod p) takes no part in the product
        if (t == 0) acc = z[0];
        else fe_mul(acc, acc, z[t]);
        if (t < K - 1) {
            if (PREFIX_IN_LDS) lds_put_fe(pre_lds + t * 10 * INV_BLOCK, INV_BLOCK, threadIdx.x, acc);
            else pre[t] = acc;
        }
    }
    // ONE inversion per QUAD of lanes (4 K elements): the pairs' products, the quad's product T, 1 / T by the four lanes together
    // (fe_invert_quad: the division steps' three pairs on three lanes, ~7 700 instructions instead of one lane's ~13 700), then
    // each lane's own 1 / acc = (1 / T) * (the other pair's product) * (its partner's product)
    fe inv;
    {
        fe partner, pair, other_pair, total;
        quad::fe_qperm<1, 0, 3, 2>(partner, acc);
        fe_mul(pair, acc, partner);
        quad::fe_qperm<2, 3, 0, 1>(other_pair, pair);
        fe_mul(total, pair, other_pair);
        fe_invert_quad(inv, total);
        fe_mul(inv, inv, other_pair);
        fe_mul(inv, inv, partner);
    }
#pragma unroll
    for (int t = K - 1; t >= 0; t--) {
        const size_t e = j + (size_t)t * m;
        fe zi;
        if (t > 0) {
            fe p;
            if (PREFIX_IN_LDS) lds_get_fe(p, pre_lds + (t - 1) * 10 * INV_BLOCK, INV_BLOCK, threadIdx.x);
            else p = pre[t - 1];
            fe_mul(zi, inv, p);
            fe_mul(inv, inv, z[t]);
        } else {
            zi = inv;
        }
        const u32 was_zero = ((zero_mask >> t) & 1u) ? 0xffffffffu : 0u;
        fe zero;
        fe_set_u32(zero, 0);
        fe_select(zi, was_zero, zero, zi);
        if (live && e < n) fin.emit(e, zi);
    }
