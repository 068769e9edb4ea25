// The body of k_dqn_reduce_adam and k_dqn_reduce_adam_slots (learner.hip includes this text into both) behind their argument
// unpacking.  In scope where it is included, under k_dqn_reduce_adam's parameter names: partials, nblk, P, stride, local, target,
// m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt, hard_update, loss, raw, go_word, go_value, img.
//
// Why text and not a function.  k_dqn_reduce_adam's instruction stream is held fixed (scripts/isa_account.py --compare; the
// baseline is profiles/isa_account_kernarg_preload.txt, the stream with the gate behind the loads), and behind a __forceinline__
// function with these parameters both kernels kept their instruction and register counts but issued the early loads of m / v / w
// in another order and moved one shift: five lines of the listing.
    // gated update (uavenv_dqn_reduce_adam_gated): the step kernel of this pass stamps go_word with go_value when it moved at
    // least one agent; a pass in which every agent had already finished leaves the learner exactly as it is (the reference's loop
    // has left run_eposide by then, Envs/PathPlan_City.py:456-459)
    //
    // The gate word is requested FIRST and tested LAST of the loads: the test stands behind the issue of every load, so that the
    // word's round trip runs under theirs instead of in front of them.  Every operand of these loads lies in the first 56 bytes of
    // k_dqn_reduce_adam's arguments, which a wavefront has in registers when it starts (kernel-argument preload); in front of the
    // loads, the test made their addresses wait for the argument fetch and then for the word.  A pass that is gated off loads and
    // drops what it loaded; the test precedes the first store, the LDS reduction included.
    UAV_HOT_PRIO();
    uint32_t go_seen = go_value;
    if (go_word) go_seen = __hip_atomic_load(go_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __shared__ float cnt_part[4];
    const int tid = (int)threadIdx.x;
    const int p = (int)blockIdx.x * 32 + tid;
    // this parameter's moments and value are requested next: their round trip runs under the partial rows' (behind the
    // reduction's barriers they were a second, dependent round trip of the launch)
    float m0 = 0.0f, v0 = 0.0f, w0 = 0.0f;
    if (tid < 32 && p < P) { m0 = m[p]; v0 = v[p]; w0 = local[p]; }
    float c;
    const floatx4 acc4 = reduce_columns_load(partials, nblk, P, stride, c);
    asm volatile("" : "+v"(go_seen));         // pin the test here: hipcc otherwise compares, and waits for the word, where it is loaded
    if (go_seen != go_value) return;
    const float t = reduce_columns_sum(acc4);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((tid & 63) == 0) cnt_part[tid >> 6] = c;
    __syncthreads();
    const float cnt = (cnt_part[0] + cnt_part[1]) + (cnt_part[2] + cnt_part[3]);
    const float inv = 1.0f / (cnt > 1.0f ? cnt : 1.0f);
    if (tid < 32 && p < P + 2) {
        if (raw) raw[p] = t;
        if (p < P) {
            const float gp = t * inv;
            const float mp = m0 + (gp - m0) * (1.0f - beta1);
            const float vp = v0 * beta2 + (1.0f - beta2) * gp * gp;
            m[p] = mp;
            v[p] = vp;
            const float np = w0 - (lr / bc1) * (mp / (sqrtf(vp) / bc2_sqrt + eps));
            local[p] = np;
            if (hard_update) target[p] = np;
            if (img) {                        // the C loop's layer-1 image follows the parameters (qnet_device.hpp: img_store_param)
                img_store_param(img, p, np);
                if (hard_update) img_store_param(img + kSplitF, p, np);
            }
        } else if (p == P && loss) {
            *loss = t * inv;
        }
    }
