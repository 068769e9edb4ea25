// The body of k_dqn_grad_packed8<GLDS> and k_dqn_grad_slots<GLDS> (learner.hip includes this text into both): a workgroup of the
// packed8 family from the LDS carve-up to the last store of its partial row.  In scope where it is included: GLDS, the GradArgs `g`,
// the Grad2Args `ga`.
//
// Why text and not a function.  The single-learner loops and the benchmark are timed on k_dqn_grad_packed8, so its instruction
// stream is held fixed (scripts/isa_account.py --compare), and every function form moved it, at unchanged register counts or
// nearly so: the whole body behind one __forceinline__ call (taking g and ga, or ga alone) came out 5 / 7 instructions longer
// (GLDS false / true); the row writer with the csum tail as a function of its own, 12 / 9 shorter; that writer plus a function
// for the accumulator clear and the tile loop, 17 / 6 shorter.  Only grad_ldsp, the carve-up, left the stream as it was.
    constexpr int NMAX = 4;
    extern __shared__ __align__(16) float lds[];
    const GradLdsP L = grad_ldsp(lds);
    float *qn_lds = lds + kPoEnd;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wv >> 2, strip = wv & 3;
    const int r = lane & 15, gq = lane >> 4;
    const int n2 = g.n_actions + (g.dueling ? 1 : 0);
    GradAcc8 A;
#pragma unroll
    for (int u = 0; u < 6; ++u) A.acc[u] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 6; ++a) A.csum[a] = 0.0f;
    L_STAMP(0);
    const int step = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    grad_tile_packed8<true, GLDS>(g, L, qn_lds, tile, tile + step < ga.n_tiles, A);
    for (tile += step; tile < ga.n_tiles; tile += step)
        grad_tile_packed8<false, GLDS>(g, L, qn_lds, tile, tile + step < ga.n_tiles, A);
    L_STAMP(5);
    // ---- the partial-gradient row of this workgroup: dW1 | db1 | dW2 | db2 | loss sum | valid count
    float *out = g.partials + (size_t)blockIdx.x * ga.stride;
    const int oW2 = kHid * kW + kHid, ob2 = oW2 + n2 * kHid;
    const int j = 16 * strip + r;
    // (round 5, measured: non-temporal stores of the row lengthen this kernel by 0.8 us and shorten the next by as much -- the 6.8 MB
    // of partial rows cross the memory system once either way)
    // (grad_products_split8's register layout) group 1: acc[u] = tile u of the flag columns (exact zeros at the scalar columns, which
    // group 0 stores from its gathered tile: columns 0..10 and 86..89 are left out here); group 0: acc[0] = the gathered tile
    // (entries 0..10 = columns 0..10, 11..14 = 86..89, 15 = db1), acc[1] = dW2^T; columns 96..99 are constant zero
    if (grp == 1) {
        float *t0 = out + j * kW + 4 * gq;
        if (gq == 3) UAV_ROW_ST4(t0, A.acc[0]);                      // columns 12..15
        else if (gq == 2) t0[3] = A.acc[0][3];                       // column 11
#pragma unroll
        for (int u = 1; u < 5; ++u) UAV_ROW_ST4(out + j * kW + 16 * u + 4 * gq, A.acc[u]);
        float *t5 = out + j * kW + 80 + 4 * gq;
        if (gq == 0 || gq == 3) UAV_ROW_ST4(t5, A.acc[5]);
        else {                                                       // columns 84, 85 (gq 1) / 90, 91 (gq 2): one 8-byte store of the chosen half
            const int h = 2 * (gq - 1);
            *reinterpret_cast<float2 *>(t5 + h) = gq == 1 ? make_float2(A.acc[5][0], A.acc[5][1]) : make_float2(A.acc[5][2], A.acc[5][3]);
        }
    } else {
        const floatx4 sc = A.acc[0];
        if (gq < 2) UAV_ROW_ST4(out + j * kW + 4 * gq, sc);                                            // columns 0..7
        else if (gq == 2) { out[j * kW + 8] = sc[0]; out[j * kW + 9] = sc[1]; out[j * kW + 10] = sc[2]; out[j * kW + 86] = sc[3]; }
        else { out[j * kW + 87] = sc[0]; out[j * kW + 88] = sc[1]; out[j * kW + 89] = sc[2]; out[kHid * kW + j] = sc[3]; }
        if (gq == 0) UAV_ROW_ST4(out + j * kW + 96, (floatx4{0.0f, 0.0f, 0.0f, 0.0f}));
        if (r < n2) UAV_ROW_ST4(out + oW2 + r * kHid + 16 * strip + 4 * gq, A.acc[1]);                  // dW2^T
    }
    if (grp == 0 && lane == 0) {
#pragma unroll
        for (int a = 0; a < NMAX + 2; ++a) L.red[strip * (kMaxOut + 2) + a] = A.csum[a];
    }
    __syncthreads();
    if (tid < NMAX + 2) {
        const float s = (L.red[tid] + L.red[(kMaxOut + 2) + tid]) + (L.red[2 * (kMaxOut + 2) + tid] + L.red[3 * (kMaxOut + 2) + tid]);
        // db2 | loss sum, valid count: one store at a chosen address (columns n2 .. NMAX - 1 of the sums belong to no output)
        float *dst = out + (tid < NMAX ? ob2 + tid : g.P + (tid - NMAX));
        if (tid < n2 || tid >= NMAX) *dst = s;
    }
