// fed.hip -- the federated merge of the per-UAV trainers (Envs/PathPlan_City.py:469-475, :590-601) on the device.
//
// Federated_Learning_AC deep-copies agent 0's actor, adds every other agent's tensors to it in agent order, and hands the
// result to every agent through replace_param (Trainer/SAC_Trainer.py:456-459).  With one flat f32 parameter block per
// trainer (sac.py: FusedSACLearner._blocks[0]; learner.py: FusedDQNLearner.flat[0]) that is one pass over U blocks: each
// thread owns four consecutive floats, reads them from every block (independent 16-byte loads, all in flight together),
// adds them in agent order -- ((w_0 + w_1) + w_2) + ..., the reference's order, so the f32 sums are bit-identical to
// torch's -- scales, and stores the result into every block.  HBM-bound: 2 x U x n x 4 bytes per call (U = 4 actors of
// 6 724 floats: 215 KB), one launch, no atomics.
//
// `scale`: the executed reference never applies its division (the `state_dict()[k] = torch.div(...)` of :597 assigns into a
// temporary dict; tests/golden/federated_ac.npz, oracle/gen_golden_federated.py), so its merge is the SUM: scale = 1 is the
// reference as executed, scale = 1 / U the mean its comment ("local平均") intends.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavenv.h"
#include "qnet_device.hpp"

namespace {

struct FedArgs {
    float *block[UAVENV_FED_MAX_BLOCKS];
    int32_t n_blocks;
    int32_t n_floats;
    float scale;
};

__global__ __launch_bounds__(256) void k_fed_aggregate(FedArgs a)
{
    const int i4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= a.n_floats) return;
    if (i4 + 4 <= a.n_floats) {
        float4 v[UAVENV_FED_MAX_BLOCKS];
#pragma unroll
        for (int j = 0; j < UAVENV_FED_MAX_BLOCKS; ++j)
            if (j < a.n_blocks) v[j] = *reinterpret_cast<const float4 *>(a.block[j] + i4);
        float4 s = v[0];
#pragma unroll
        for (int j = 1; j < UAVENV_FED_MAX_BLOCKS; ++j)
            if (j < a.n_blocks) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
        if (a.scale != 1.0f) { s.x *= a.scale; s.y *= a.scale; s.z *= a.scale; s.w *= a.scale; }
#pragma unroll
        for (int j = 0; j < UAVENV_FED_MAX_BLOCKS; ++j)
            if (j < a.n_blocks) *reinterpret_cast<float4 *>(a.block[j] + i4) = s;
    } else {
        for (int i = i4; i < a.n_floats; ++i) {
            float s = a.block[0][i];
            for (int j = 1; j < a.n_blocks; ++j) s += a.block[j][i];
            if (a.scale != 1.0f) s *= a.scale;
            for (int j = 0; j < a.n_blocks; ++j) a.block[j][i] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Federated_Learning_choice (Envs/PathPlan_City.py:644-684), the DQN-family merge the reference executes: for p = 0 .. U-1 IN
// ORDER, each step on the blocks as the earlier steps left them, UAV p forwards 10 of its own replayed states through its
// q_local and through every other UAV's, takes the (U-1)//2 others whose Q-values are closest (MSELoss over all S x A
// elements, stable sort), and becomes the f32 mean of itself and those -- adds in chosen order, then a true division.
//
// ONE launch of ONE 256-thread workgroup: U^2 forwards of <= 16 rows and U merges of <= 8 x ~7 k floats, strictly sequential
// in p.  All four wavefronts sit on one CU, so the blocks step p writes reach step p + 1's loads through workgroup barriers
// alone.  Every parameter load is a per-lane vector load (w_issue, the fc2 staging below, the merge): none goes through the
// scalar cache, which those barriers do not cover.  The net pointers are copied into LDS first, so that indexing them by a
// chosen index is an LDS read and not a dynamically indexed kernel argument.
// Per (p, j): all threads stage net j's fc1 (+ b1 as column 100) and fc2 into LDS, wavefront 0 runs the 16-row strip
// (lane & 15 = state; fwd_strip_packed + q_strip: the f32 MFMA forward) and leaves per-row sums of squared differences; thread
// 0 then sums them in row order, sorts, and all threads merge.
struct FedChoiceArgs {
    const uint32_t *obs;          // [frames][n_agents][20 dwords]
    const int32_t *pairs;         // [n_nets][n_states][2]
    float *local[UAVENV_DQN_MAX_SLOTS];
    float *dist_out;              // nullable [n_nets][n_nets]
    int32_t *chosen_out;          // nullable [n_nets][n_nets]
    int32_t *status_out;
    int32_t frames, n_agents, n_states, n_nets, n_actions, dueling, n_params;
};

template <int NMAX>
__global__ __launch_bounds__(256) void k_fed_choice(FedChoiceArgs g)
{
    using namespace uavq;
    __shared__ __align__(16) float W1[kTileF];                     // fc1 | b1 of the net being forwarded
    __shared__ __align__(16) float W2[kMaxOut * kHid];
    __shared__ __align__(16) float b2[kMaxOut];
    __shared__ float qp[16 * kMaxOut];                             // q_local_p(states_p)
    __shared__ float rsum[UAVENV_DQN_MAX_SLOTS * 16];              // [j][state]: sum_a (q_p - q_j)^2
    __shared__ float dist[UAVENV_DQN_MAX_SLOTS];
    __shared__ float *ptr[UAVENV_DQN_MAX_SLOTS];
    __shared__ int order[UAVENV_DQN_MAX_SLOTS];
    __shared__ int bad;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15;
    const int U = g.n_nets, S = g.n_states, A = g.n_actions;
    const int n2 = A + (g.dueling ? 1 : 0);
    const int k = (U - 1) / 2;
    if (tid == 0) bad = 0;
    if (tid < UAVENV_DQN_MAX_SLOTS) ptr[tid] = g.local[tid];
    __syncthreads();
    for (int i = tid; i < U * S; i += 256) {
        const int f = g.pairs[2 * i], a = g.pairs[2 * i + 1];
        if (f < 0 || f >= g.frames || a < 0 || a >= g.n_agents) bad = 1;
    }
    __syncthreads();
    if (bad) {                                                     // an out-of-range index never becomes an address
        if (tid == 0) *g.status_out = 1;
        return;
    }
    if (tid == 0) *g.status_out = 0;
    for (int p = 0; p < U; ++p) {
        PRow R;
        {
            const int i = p * S + (r < S ? r : 0);
            const int f = g.pairs[2 * i], a = g.pairs[2 * i + 1];
            prow_load(R, g.obs + ((size_t)f * (size_t)g.n_agents + (size_t)a) * kPackedDwords);
        }
        for (int jj = 0; jj < U; ++jj) {
            const int j = jj == 0 ? p : (jj <= p ? jj - 1 : jj);    // p itself first, then the others in index order
            const NetDev nl = net_view(ptr[j], n2);
            {
                floatx4 vW[kStageIters];
                w_issue(vW, nl.W1);
                const float pb1 = nl.b1[tid < kHid ? tid : kHid - 1];
                float pw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) pw[q] = nl.W2[tid + 256 * q < n2 * kHid ? tid + 256 * q : 0];
                const float pb2 = nl.b2[tid < n2 ? tid : 0];
                w_commit(W1, vW, pb1);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (tid + 256 * q < n2 * kHid) W2[tid + 256 * q] = pw[q];
                if (tid < n2) b2[tid] = pb2;
            }
            __syncthreads();
            if (wv == 0) {
                floatx4 h[4];
                fwd_strip_packed(W1, R, h);
                float q[NMAX];
                W2Frag<NMAX> F;
                w2_load<NMAX>(F, W2, b2, n2);
                q_strip<NMAX>(h, F, n2, A, g.dueling, q);
                if (lane < 16) {
                    if (jj == 0) {
#pragma unroll
                        for (int a = 0; a < NMAX; ++a) qp[r * kMaxOut + a] = q[a];
                    } else {
                        float e = 0.0f;
#pragma unroll
                        for (int a = 0; a < NMAX; ++a)
                            if (a < A) { const float d = qp[r * kMaxOut + a] - q[a]; e += d * d; }
                        rsum[j * 16 + r] = e;
                    }
                }
            }
            __syncthreads();                                        // the tiles are restaged; rsum is read by thread 0
        }
        if (tid == 0) {
            int n = 0;
            for (int j = 0; j < U; ++j) {
                float d = 0.0f;
                if (j != p) {
                    for (int s = 0; s < S; ++s) d += rsum[j * 16 + s];
                    d /= (float)(S * A);                            // MSELoss: the mean over all S x A elements
                    int pos = n++;                                  // stable insertion under <: ties keep the index order
                    for (; pos > 0 && d < dist[order[pos - 1]]; --pos) order[pos] = order[pos - 1];
                    order[pos] = j;
                }
                dist[j] = d;
                if (g.dist_out) g.dist_out[p * U + j] = d;
            }
            if (g.chosen_out)
                for (int c = 0; c < U; ++c) g.chosen_out[p * U + c] = c < k ? order[c] : -1;
        }
        __syncthreads();
        if (k > 0) {
            float *wp = ptr[p];
            const float div = (float)(k + 1);
            for (int i = tid; i < g.n_params / 4; i += 256) {
                floatx4 t = *reinterpret_cast<const floatx4 *>(wp + 4 * i);
                for (int c = 0; c < k; ++c) t += *reinterpret_cast<const floatx4 *>(ptr[order[c]] + 4 * i);
                *reinterpret_cast<floatx4 *>(wp + 4 * i) = t / div;
            }
            const int i = (g.n_params & ~3) + tid;
            if (i < g.n_params) {
                float t = wp[i];
                for (int c = 0; c < k; ++c) t += ptr[order[c]][i];
                wp[i] = t / div;
            }
        }
        __syncthreads();                                            // step p + 1 stages what this step wrote
    }
}

}  // namespace

extern "C" int uavenv_fed_choice(const void *obs_dev, int32_t frames, int32_t n_agents, const int32_t *pairs_dev, int32_t n_states,
                                 const UavDqnNet *const *nets, int32_t n_nets, float *dist_out_dev, int32_t *chosen_out_dev,
                                 int32_t *status_out_dev, void *stream)
{
    using namespace uavq;
    if (!nets || n_nets < 1 || n_nets > UAVENV_DQN_MAX_SLOTS || n_states < 1 || n_states > 16) return UAVENV_EINVAL;
    if (!obs_dev || !pairs_dev || !status_out_dev || frames <= 0 || n_agents <= 0 || (((uintptr_t)obs_dev) & 15u) != 0) return UAVENV_EINVAL;
    FedChoiceArgs g;
    for (int j = 0; j < UAVENV_DQN_MAX_SLOTS; ++j) g.local[j] = nullptr;
    for (int j = 0; j < n_nets; ++j) {
        const UavDqnNet *n = nets[j];
        if (!n || !n->local || n->w != kW || n->hid != kHid || n->n_actions < 2 ||
            n->n_actions + (n->dueling ? 1 : 0) + 2 > kMaxOut)      // the heads uavenv_dqn_act_slots takes
            return UAVENV_EINVAL;
        if (n->mfma_dtype != UAVENV_MFMA_F32 || (((uintptr_t)n->local) & 15u) != 0) return UAVENV_EINVAL;
        if (n->n_actions != nets[0]->n_actions || (n->dueling != 0) != (nets[0]->dueling != 0)) return UAVENV_EINVAL;
        for (int i = 0; i < j; ++i)                                 // a net merged into itself would race with itself
            if (nets[i]->local == n->local) return UAVENV_EINVAL;
        g.local[j] = n->local;
    }
    g.obs = reinterpret_cast<const uint32_t *>(obs_dev); g.pairs = pairs_dev;
    g.dist_out = dist_out_dev; g.chosen_out = chosen_out_dev; g.status_out = status_out_dev;
    g.frames = frames; g.n_agents = n_agents; g.n_states = n_states; g.n_nets = n_nets;
    g.n_actions = nets[0]->n_actions; g.dueling = nets[0]->dueling ? 1 : 0;
    const int n2 = g.n_actions + g.dueling;
    g.n_params = kHid * kW + kHid + n2 * kHid + n2;
    if (n2 <= 4) hipLaunchKernelGGL(k_fed_choice<4>, dim3(1), dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((k_fed_choice<kMaxOut - 2>), dim3(1), dim3(256), 0, (hipStream_t)stream, g);
    return hipGetLastError() == hipSuccess ? UAVENV_OK : UAVENV_EHIP;
}

extern "C" int uavenv_fed_aggregate(float *const *blocks_dev, int32_t n_blocks, int32_t n_floats, float scale, void *stream)
{
    if (!blocks_dev || n_blocks <= 0 || n_blocks > UAVENV_FED_MAX_BLOCKS || n_floats <= 0) return UAVENV_EINVAL;
    FedArgs a;
    for (int j = 0; j < UAVENV_FED_MAX_BLOCKS; ++j) a.block[j] = nullptr;
    for (int j = 0; j < n_blocks; ++j) {
        if (!blocks_dev[j] || ((uintptr_t)blocks_dev[j] & 15u) != 0) return UAVENV_EINVAL;
        for (int k = 0; k < j; ++k)                               // two trainers sharing a block would race with themselves
            if (blocks_dev[k] == blocks_dev[j]) return UAVENV_EINVAL;
        a.block[j] = blocks_dev[j];
    }
    a.n_blocks = n_blocks;
    a.n_floats = n_floats;
    a.scale = scale;
    const int threads = (n_floats + 3) / 4;
    hipLaunchKernelGGL(k_fed_aggregate, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? UAVENV_OK : UAVENV_EHIP;
}
