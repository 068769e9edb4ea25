// p2p.hip -- one-shot all-reduce of the learner's ~26 KB gradient bucket over peer-mapped HBM (xGMI), on the stream.
//
// The multi-GPU loop is strictly ordered (act -> step -> learn -> act: the next action needs the updated weights), so
// the gradient exchange sits on the critical path of every ~40 us pass.  A collective through torch.distributed / RCCL
// costs a host round trip plus 20-40 us of ring latency for a message this small.  Here every rank owns a receive area
// in uncached device memory that its peers map through HIP IPC:
//     push   (tail of the gradient reduction) each workgroup stores its 32 column sums straight into slot [my rank] of
//            EVERY rank's receive area (its own included);
//     pull   (head of the Adam kernel, the next launch on the stream) raises flag [my rank] = seq at every rank
//            (system-scope release), then one thread per workgroup waits until all `world` flags of its own rank show
//            seq (system-scope loads of local memory), then every thread adds the `world` slots IN RANK ORDER -- all
//            ranks therefore apply bit-identical updates -- and Adam runs as in k_dqn_adam.
// Two alternating slots per rank (seq parity): a rank can be at most one update ahead of a peer, because its next push
// is enqueued behind its own pull of the current one.  xGMI is point to point: 7 peers x 26 KB out and in per rank and
// update, one hop, no ring.
//
// Failure handling.  Every wait is bounded.  A timeout sets a STICKY error word (host-mapped, so the host reads it
// without synchronising): the pull that timed out and every later one skip the Adam step -- the rank's weights freeze
// instead of being stepped with stale or half-written slots -- and uavenv_dqn_reduce_p2p / uavenv_dqn_adam_p2p /
// uavenv_loop_run return UAVENV_EP2P from then on, so the caller can fall back to the collective (csrc/coll.hip) and
// re-broadcast the weights.  Every `check_every` updates the Adam kernels fold a 64-bit checksum of the new weights'
// bit patterns into the next bucket; a rank whose peers report a different checksum raises the same sticky error
// (code UAVENV_P2P_ERR_DIVERGED): the ranks are bit-identical by construction and this is how a violation shows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <new>
#include <vector>

#include "../../include/uavenv.h"
#include "uavenv_device.hpp"
#include "qnet_device.hpp"
#include "dqn_internal.hpp"

namespace {
constexpr int kMaxWorld = 16;
constexpr size_t kFlagBytes = (size_t)(kMaxWorld + 1) * 64;   // one 64-byte line per peer flag + one for this rank's verdict word
constexpr uint32_t kSpinLimit = 1u << 24;            // x ~0.25 us per poll: about four seconds (uavenv_p2p_configure changes it)
}

struct UavP2P {
    int world = 0, rank = 0, bucket = 0, bucket_pad = 0;
    size_t bytes = 0;
    unsigned char *local = nullptr;                   // [flags: kMaxWorld x 64 B][verdict: 64 B][recv: world x 2 x bucket_pad floats]
    unsigned char *peer[kMaxWorld] = {nullptr};       // peer[r] = rank r's area as mapped here (peer[rank] = local)
    bool opened[kMaxWorld] = {false};
    unsigned long long *wsum = nullptr;               // [2] weight checksums (device memory), by parity of the check index
    uint32_t *errors = nullptr;                       // device: [0] timeouts, [1] sticky error code, [2] checksum mismatches
    float *check_buf = nullptr;                       // device: four floats (16-byte aligned): the words uavenv_p2p_check_blocks pushes
    volatile uint32_t *host_code = nullptr;           // host-mapped copy of the sticky code (polled without synchronising)
    uint32_t *host_code_dev = nullptr;                // its device address
    uint32_t seq = 0;
    uint32_t spin_limit = kSpinLimit;
    int carry_cur = -1, pending_idx = 0;
    uint32_t check_every = 256;                       // 0 = never
    uint32_t n_checks = 0;                            // checksums folded so far
    bool check_pending = false;                       // the last Adam folded a checksum: the next push carries it
    bool connected = false;
};

namespace {

struct P2PDev {
    unsigned char *peer[kMaxWorld];
    int world, rank, bucket_pad;
    uint32_t seq;
    unsigned long long *wsum;                         // [2]
    uint32_t *errors;                                 // [0] timeouts, [1] sticky code, [2] mismatches
    uint32_t *host_code;                              // host-mapped copy of [1]
    uint32_t spin_limit;
    int carry, fold;                                  // push: carry wsum[carry] (or -1); pull: fold into wsum[fold] (or -1)
};

__device__ __forceinline__ float *recv_slot(unsigned char *area, int from, uint32_t seq, int bucket_pad)
{
    return reinterpret_cast<float *>(area + kFlagBytes) + ((size_t)from * 2 + (seq & 1u)) * (size_t)bucket_pad;
}

__device__ __forceinline__ uint32_t *flag_of(unsigned char *area, int from)
{
    return reinterpret_cast<uint32_t *>(area + (size_t)from * 64);
}

// The wait of a pull launch, DECIDED ONCE: workgroup 0 waits for the `world` flags (bounded), compares the weight checksums
// when the bucket carries them, and publishes (seq, verdict) in this rank's verdict word (uncached, like the flags); every
// other workgroup takes that verdict.  (Round 3 let every workgroup run its own bounded wait: a flag arriving between two
// workgroups' deadlines summed / stepped some columns and not others -- ADVICE r3.)  A workgroup that never sees workgroup
// 0's verdict (it cannot happen short of a dead launch; the bound is twice workgroup 0's own) reports a timeout itself.
// Returns 0 or the error code; thread 0 only.
__device__ uint32_t p2p_wait_once(const P2PDev &d, unsigned char *mine, int P_checksum)
{
    uint32_t *verdict = reinterpret_cast<uint32_t *>(mine + (size_t)kMaxWorld * 64);
    const uint32_t tag = d.seq << 2;
    if (blockIdx.x != 0) {
        // The sticky word first: a pull behind a REFUSED push (uavenv_dqn_reduce_p2p returns UAVENV_EP2P and uses no sequence
        // number) carries the sequence number of the last pull, whose healthy verdict is still in the verdict word -- taken from
        // there, every workgroup but the first stepped its parameters with that pull's sums once more.
        const uint32_t sticky = __hip_atomic_load(d.errors + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sticky) return sticky;
        // twice workgroup 0's own worst case (world waits of spin_limit polls each), in 64 bits -- 2 * 2^27 * 16 wrapped a
        // uint32 to ~1 k polls and raised a spurious sticky timeout -- and at workgroup 0's poll interval
        const unsigned long long bound = 2ull * (unsigned long long)d.spin_limit * (unsigned long long)d.world + 1024ull;
        unsigned long long spins = 0;
        uint32_t v;
        while (((v = __hip_atomic_load(verdict, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM)) & ~3u) != tag) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > bound) {
                __hip_atomic_fetch_add(d.errors, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(d.errors + 1, (uint32_t)UAVENV_P2P_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(d.host_code, (uint32_t)UAVENV_P2P_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return UAVENV_P2P_ERR_TIMEOUT;
            }
        }
        return v & 3u;
    }
    uint32_t bad = __hip_atomic_load(d.errors + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // sticky
    for (int r = 0; r < d.world && !bad; ++r) {
        uint32_t spins = 0;
        while ((int32_t)(__hip_atomic_load(flag_of(mine, r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - d.seq) < 0) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > d.spin_limit) {
                __hip_atomic_fetch_add(d.errors, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(d.errors + 1, (uint32_t)UAVENV_P2P_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(d.host_code, (uint32_t)UAVENV_P2P_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                bad = UAVENV_P2P_ERR_TIMEOUT;
                break;
            }
        }
    }
    __threadfence_system();
    if (!bad && d.carry >= 0 && P_checksum >= 0) {     // every rank folded a checksum of its weights into this bucket: all equal?
        const uint32_t *s0 = reinterpret_cast<const uint32_t *>(recv_slot(mine, 0, d.seq, d.bucket_pad));
        const uint32_t lo = __hip_atomic_load(s0 + P_checksum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t hi = __hip_atomic_load(s0 + P_checksum + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (int r = 1; r < d.world; ++r) {
            const uint32_t *sr = reinterpret_cast<const uint32_t *>(recv_slot(mine, r, d.seq, d.bucket_pad));
            if (__hip_atomic_load(sr + P_checksum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != lo ||
                __hip_atomic_load(sr + P_checksum + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != hi)
                bad = UAVENV_P2P_ERR_DIVERGED;
        }
        if (bad) {
            __hip_atomic_fetch_add(d.errors + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d.errors + 1, (uint32_t)UAVENV_P2P_ERR_DIVERGED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d.host_code, (uint32_t)UAVENV_P2P_ERR_DIVERGED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __hip_atomic_store(verdict, tag | (bad & 3u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return bad;
}

// column sums of the partial rows (as k_dqn_reduce) -> slot [rank] of every rank's receive area
__global__ void __launch_bounds__(256) k_p2p_reduce_push(const float *__restrict__ partials, int nblk, int P, int stride, P2PDev d)
{
    __shared__ float red[32][33];
    __shared__ float red2[8][33];
    const int tid = (int)threadIdx.x;
    const int cg = tid & 7, rg = tid >> 3;
    const int p4 = (int)blockIdx.x * 32 + cg * 4;
    const bool col_ok = p4 < stride;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b0 = 0; b0 < nblk; b0 += 256) {
        float4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int b = b0 + rg + 32 * k;
            t[k] = *reinterpret_cast<const float4 *>(partials + (size_t)(b < nblk ? b : nblk - 1) * stride + (col_ok ? p4 : 0));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool ok = b0 + rg + 32 * k < nblk;
            acc[0] += ok ? t[k].x : 0.0f; acc[1] += ok ? t[k].y : 0.0f;
            acc[2] += ok ? t[k].z : 0.0f; acc[3] += ok ? t[k].w : 0.0f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rg][cg * 4 + e] = acc[e];
    __syncthreads();
    {
        const int px = tid & 31, part = tid >> 5;
        red2[part][px] = (red[4 * part][px] + red[4 * part + 1][px]) + (red[4 * part + 2][px] + red[4 * part + 3][px]);
    }
    __syncthreads();
    // Eight lanes, four columns each: ONE 16-byte store per lane and peer (a receive area is uncached memory: a 4-byte store
    // is one fabric write of its own, six times the time per byte of a 16-byte one; round 2 issued 32 of them per peer here
    // and every thread of the workgroup fenced afterwards: 14.5 us against 4.8 us for the local reduction).
    // Words P + 2, P + 3 of the bucket carry the checksum of the weights the previous Adam left (bit pattern, never touched
    // by arithmetic), or zeros; the accumulator the NEXT fold will use is cleared by the lane that owns word P + 2 (its last
    // reader was the push before this one).  Columns past P + 3 are stored as zeros.
    if (tid < 8) {
        const int p0 = (int)blockIdx.x * 32 + 4 * tid;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += red2[k][4 * tid + e];
            o[e] = p0 + e < P + 2 ? t : 0.0f;
        }
        if (p0 <= P + 3 && p0 + 3 >= P + 2) {
            unsigned long long w = 0ull;
            if (d.carry >= 0) {
                w = __hip_atomic_load(d.wsum + d.carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (p0 <= P + 2) __hip_atomic_store(d.wsum + (d.carry ^ 1), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (p0 + e == P + 2) o[e] = __uint_as_float((uint32_t)w);
                if (p0 + e == P + 3) o[e] = __uint_as_float((uint32_t)(w >> 32));
            }
        }
        const float4 v4 = make_float4(o[0], o[1], o[2], o[3]);
        for (int r = 0; r < d.world; ++r)                                        // 128 B per workgroup and peer
            *reinterpret_cast<float4 *>(recv_slot(d.peer[r], d.rank, d.seq, d.bucket_pad) + p0) = v4;
        __threadfence_system();          // (the flags are raised by the NEXT launch on the stream; this is belt and braces)
    }
}

// wait for the `world` flags, add the slots in rank order, Adam (k_dqn_adam's arithmetic)
__global__ void __launch_bounds__(256) k_p2p_pull_adam(P2PDev d, float *__restrict__ local, float *__restrict__ target,
                                                       float *__restrict__ m, float *__restrict__ v, float *__restrict__ raw_out,
                                                       int P, float lr, float beta1, float beta2, float eps, float bc1,
                                                       float bc2_sqrt, int hard_update, float *__restrict__ loss, float *__restrict__ img)
{
    unsigned char *mine = d.peer[d.rank];
    // Raise flag [rank] = seq at every rank first: this kernel is launched behind k_p2p_reduce_push on the stream, so the
    // kernel boundary orders the flags after every push workgroup's stores.  (Counting the 213 push workgroups out with a
    // device-scope ticket instead -- "the last one publishes" -- serialises 213 atomics across the 8 XCDs' L2s, ~140 ns
    // each, DESIGN 3.4: most of what the exchange added to a pass.)
    if (blockIdx.x == 0 && (int)threadIdx.x < d.world) {
        __threadfence_system();
        __hip_atomic_store(flag_of(d.peer[threadIdx.x], d.rank), d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __shared__ uint32_t s_bad;
    __shared__ unsigned long long s_sum;
    // this parameter's moments and value: requested before the wait, so their round trip runs under it
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    float m0 = 0.0f, v0 = 0.0f, w0 = 0.0f;
    if (p < P && local) { m0 = m[p]; v0 = v[p]; w0 = local[p]; }
    if (threadIdx.x == 0) {
        const uint32_t bad = p2p_wait_once(d, mine, P + 2);
        __threadfence_system();
        s_bad = bad;
        s_sum = 0ull;
    }
    __syncthreads();
    const bool frozen = s_bad != 0;              // the sums below may be stale: report them, never step with them
    float cnt = 0.0f, lsum = 0.0f;
    for (int r = 0; r < d.world; ++r) {
        const float *slot = recv_slot(mine, r, d.seq, d.bucket_pad);
        cnt += __hip_atomic_load(slot + P + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        lsum += __hip_atomic_load(slot + P, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const float inv = 1.0f / (cnt > 1.0f ? cnt : 1.0f);
    if (p == 0 && loss && !frozen) *loss = lsum * inv;
    if (p == 0 && raw_out) { raw_out[P] = lsum; raw_out[P + 1] = cnt; }
    float np = 0.0f;
    if (p < P) {
        float gsum = 0.0f;
        for (int r = 0; r < d.world; ++r)
            gsum += __hip_atomic_load(recv_slot(mine, r, d.seq, d.bucket_pad) + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (raw_out) raw_out[p] = gsum;
        if (local) {                                                             // (NULL: sum only, self-test)
            np = w0;
            if (!frozen) {
                const float gp = gsum * inv;
                const float mp = m0 + (gp - m0) * (1.0f - beta1);
                const float vp = v0 * beta2 + (1.0f - beta2) * gp * gp;
                m[p] = mp;
                v[p] = vp;
                np = np - (lr / bc1) * (mp / (sqrtf(vp) / bc2_sqrt + eps));
                local[p] = np;
                if (hard_update) target[p] = np;
                if (img) {                   // the C loop's layer-1 image follows the parameters (csrc/dqn_internal.hpp)
                    uavq::img_store_param(img, p, np);
                    if (hard_update) uavq::img_store_param(img + uavq::kSplitF, p, np);
                }
            }
        }
    }
    if (d.fold >= 0 && local) {                  // checksum of the weights after this step: sum over p of mix(bits, p)
        unsigned long long h = 0ull;
        if (p < P) {
            unsigned long long x = ((unsigned long long)__float_as_uint(np) << 20) ^ (unsigned long long)(p + 1) * 0x9E3779B97F4A7C15ull;
            x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
            h = x;
        }
        atomicAdd(&s_sum, h);                    // LDS
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(d.wsum + d.fold, s_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the same exchange for ANY float buffer (the SAC learners' per-phase gradient rows, csrc/sac.hip): push = copy this
// rank's buffer into slot [rank] of every rank's receive area (16-byte stores), pull = raise the flags, wait, add the slots IN
// RANK ORDER back into the buffer.  On a sticky error the buffer is left as it was (this rank's own sums) and the host call
// returns UAVENV_EP2P: the caller must stop stepping and re-synchronise parameters and moments from one rank.
__global__ void __launch_bounds__(256) k_p2p_push(const float *__restrict__ buf, int count4, P2PDev d)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < count4) {
        const float4 v = reinterpret_cast<const float4 *>(buf)[i];
        for (int r = 0; r < d.world; ++r)
            reinterpret_cast<float4 *>(recv_slot(d.peer[r], d.rank, d.seq, d.bucket_pad))[i] = v;
    }
    __threadfence_system();
}

__global__ void __launch_bounds__(256) k_p2p_pull_sum(P2PDev d, float *__restrict__ buf, int count)
{
    unsigned char *mine = d.peer[d.rank];
    if (blockIdx.x == 0 && (int)threadIdx.x < d.world) {     // behind k_p2p_push on the stream: the boundary orders the flags after its stores
        __threadfence_system();
        __hip_atomic_store(flag_of(d.peer[threadIdx.x], d.rank), d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) {
        const uint32_t bad = p2p_wait_once(d, mine, -1);
        __threadfence_system();
        s_bad = bad;
    }
    __syncthreads();
    if (s_bad) return;
    // four floats per thread and trip (the loads of a trip independent and in flight together), a grid-stride walk: the grid is
    // capped (uavenv_p2p_allreduce) so that the workgroups WAITING above never cover the chip
    const int count4 = count >> 2;
    for (int q = (int)(blockIdx.x * blockDim.x + threadIdx.x); q < count4; q += (int)(gridDim.x * blockDim.x)) {
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int r = 0; r < d.world; ++r) {
            const float *src = recv_slot(mine, r, d.seq, d.bucket_pad) + 4 * q;
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = __hip_atomic_load(src + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += t[e];
        }
        *reinterpret_cast<float4 *>(buf + 4 * q) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
}

// ---- weight checksums for the generic exchange (the SAC learners: their buckets are plain gradient rows with no room for the
// DQN bucket's checksum words).  Every rank hashes the bit patterns of its parameter blocks (k_p2p_hash_blocks: 64-bit, order
// independent, position mixed in), pushes the two words to every rank and compares the `world` pairs on the device -- the
// compare is p2p_wait_once's, so a difference raises the same sticky error (UAVENV_P2P_ERR_DIVERGED) through the same words.
struct HashBlocks {
    const float *block[UAVENV_P2P_CHECK_MAX_BLOCKS];
    int32_t n_floats[UAVENV_P2P_CHECK_MAX_BLOCKS];
    int32_t n_blocks;
};

__global__ void __launch_bounds__(256) k_p2p_hash_blocks(HashBlocks h, unsigned long long *acc)
{
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    const int b = (int)blockIdx.y;
    unsigned long long mine = 0ull;
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < h.n_floats[b]; p += (int)(gridDim.x * blockDim.x)) {
        unsigned long long x = ((unsigned long long)__float_as_uint(h.block[b][p]) << 20) ^
                               ((unsigned long long)(p + 1) + ((unsigned long long)(b + 1) << 40)) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        mine += x;
    }
    atomicAdd(&s_sum, mine);                     // LDS
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) __hip_atomic_fetch_add(acc, s_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// acc -> four floats holding its two words as bit patterns (what k_p2p_push sends), acc <- 0 for the next check
__global__ void k_p2p_hash_words(unsigned long long *acc, float *buf4)
{
    const unsigned long long w = *acc;
    buf4[0] = __uint_as_float((uint32_t)w);
    buf4[1] = __uint_as_float((uint32_t)(w >> 32));
    buf4[2] = 0.0f; buf4[3] = 0.0f;
    *acc = 0ull;
}

__global__ void __launch_bounds__(64) k_p2p_pull_check(P2PDev d)
{
    unsigned char *mine = d.peer[d.rank];
    if (blockIdx.x == 0 && (int)threadIdx.x < d.world) {     // behind k_p2p_push on the stream
        __threadfence_system();
        __hip_atomic_store(flag_of(d.peer[threadIdx.x], d.rank), d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) (void)p2p_wait_once(d, mine, 0);    // words 0 / 1 of every rank's slot must agree
}

P2PDev dev_view(const UavP2P *c, int carry, int fold)
{
    P2PDev d;
    for (int r = 0; r < kMaxWorld; ++r) d.peer[r] = c->peer[r];
    d.world = c->world; d.rank = c->rank; d.bucket_pad = c->bucket_pad; d.seq = c->seq;
    d.wsum = c->wsum; d.errors = c->errors; d.host_code = c->host_code_dev; d.spin_limit = c->spin_limit;
    d.carry = carry; d.fold = fold;
    return d;
}

}  // namespace

extern "C" {

int uavenv_p2p_create(int32_t world, int32_t rank, int32_t bucket_floats, UavP2P **out)
{
    if (!out || world < 1 || world > kMaxWorld || rank < 0 || rank >= world || bucket_floats <= 0) return UAVENV_EINVAL;
    UavP2P *c = new (std::nothrow) UavP2P();
    if (!c) return UAVENV_ENOMEM;
    c->world = world; c->rank = rank; c->bucket = bucket_floats;
    c->bucket_pad = (bucket_floats + 2 + 63) & ~63;           // + the two checksum words
    c->bytes = kFlagBytes + (size_t)world * 2 * c->bucket_pad * sizeof(float);
    // uncached: peers write it while this device reads it inside running kernels
    if (hipExtMallocWithFlags((void **)&c->local, c->bytes, hipDeviceMallocUncached) != hipSuccess) { delete c; return UAVENV_ENOMEM; }
    if (hipMalloc((void **)&c->wsum, 2 * sizeof(unsigned long long) + 4 * sizeof(uint32_t) + 4 * sizeof(float)) != hipSuccess) {
        (void)hipFree(c->local); delete c; return UAVENV_ENOMEM;
    }
    c->errors = reinterpret_cast<uint32_t *>(c->wsum + 2);
    c->check_buf = reinterpret_cast<float *>(c->errors + 4);          // (byte offset 32 of a hipMalloc block: 16-byte aligned)
    // the sticky error code also lands in host-mapped memory: the host polls it without synchronising
    if (hipHostMalloc((void **)&c->host_code, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->host_code_dev, (void *)c->host_code, 0) != hipSuccess) {
        if (c->host_code) (void)hipHostFree((void *)c->host_code);
        (void)hipFree(c->local); (void)hipFree(c->wsum); delete c; return UAVENV_ENOMEM;
    }
    *c->host_code = 0;
    (void)hipMemset(c->local, 0, c->bytes);
    (void)hipMemset(c->wsum, 0, 2 * sizeof(unsigned long long) + 4 * sizeof(uint32_t) + 4 * sizeof(float));
    (void)hipDeviceSynchronize();
    c->peer[rank] = c->local;
    c->connected = world == 1;
    *out = c;
    return UAVENV_OK;
}

int uavenv_p2p_configure(UavP2P *c, int32_t check_every, int32_t spin_limit)
{
    if (!c || check_every < 0 || spin_limit < 0) return UAVENV_EINVAL;
    c->check_every = (uint32_t)check_every;
    if (spin_limit > 0) c->spin_limit = (uint32_t)spin_limit;
    return UAVENV_OK;
}

int uavenv_p2p_handle(UavP2P *c, void *handle_out)
{
    if (!c || !handle_out) return UAVENV_EINVAL;
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, c->local) != hipSuccess) return UAVENV_EHIP;
    static_assert(sizeof(hipIpcMemHandle_t) <= UAVENV_P2P_HANDLE_BYTES, "IPC handle size");
    memset(handle_out, 0, UAVENV_P2P_HANDLE_BYTES);
    memcpy(handle_out, &h, sizeof(h));
    return UAVENV_OK;
}

int uavenv_p2p_can_reach(int32_t device, int32_t peer_device)
{
    if (device == peer_device) return 1;
    int ok = 0;
    if (hipDeviceCanAccessPeer(&ok, device, peer_device) != hipSuccess) return 0;
    return ok ? 1 : 0;
}

int uavenv_p2p_connect(UavP2P *c, const void *all_handles)
{
    if (!c || !all_handles) return UAVENV_EINVAL;
    for (int r = 0; r < c->world; ++r) {
        if (r == c->rank) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, (const unsigned char *)all_handles + (size_t)r * UAVENV_P2P_HANDLE_BYTES, sizeof(h));
        void *p = nullptr;
        if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) return UAVENV_EHIP;
        c->peer[r] = (unsigned char *)p;
        c->opened[r] = true;
    }
    c->connected = true;
    return UAVENV_OK;
}

int uavenv_p2p_destroy(UavP2P *c)
{
    if (!c) return UAVENV_OK;
    (void)hipDeviceSynchronize();
    for (int r = 0; r < c->world; ++r)
        if (c->opened[r]) (void)hipIpcCloseMemHandle(c->peer[r]);
    (void)hipFree(c->local);
    (void)hipFree(c->wsum);
    if (c->host_code) (void)hipHostFree((void *)c->host_code);
    delete c;
    return UAVENV_OK;
}

const uint32_t *uavenv_p2p_error_word(const UavP2P *c)
{
    return c ? c->errors + 1 : nullptr;
}

int uavenv_p2p_errors(UavP2P *c, int32_t *timeouts_out)
{
    if (!c || !timeouts_out) return UAVENV_EINVAL;
    uint32_t e = 0;
    if (hipMemcpy(&e, c->errors, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return UAVENV_EHIP;
    *timeouts_out = (int32_t)e;
    return UAVENV_OK;
}

int uavenv_p2p_status(UavP2P *c, int32_t synchronise, int32_t *out4)
{
    if (!c || !out4) return UAVENV_EINVAL;
    out4[0] = (int32_t)*c->host_code;                          // sticky code as the host sees it right now
    out4[1] = out4[2] = -1;
    out4[3] = (int32_t)c->n_checks;
    if (synchronise) {
        uint32_t e[3] = {0, 0, 0};
        if (hipMemcpy(e, c->errors, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return UAVENV_EHIP;
        out4[0] = (int32_t)e[1]; out4[1] = (int32_t)e[0]; out4[2] = (int32_t)e[2];
    }
    return UAVENV_OK;
}

int uavenv_p2p_inject_fault(UavP2P *c, int32_t code)
{
    if (!c || code < 0) return UAVENV_EINVAL;
    const uint32_t v = (uint32_t)code;
    if (hipMemcpy(c->errors + 1, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess) return UAVENV_EHIP;
    *c->host_code = v;
    return UAVENV_OK;
}

int uavenv_dqn_reduce_p2p(const UavDqnNet *net, const float *partials, int32_t n_partials, UavP2P *c, void *stream)
{
    if (!net || !partials || n_partials <= 0 || !c || !c->connected) return UAVENV_EINVAL;
    const int P = uavenv_dqn_num_params(net);
    if (P <= 0 || P + 2 > c->bucket) return UAVENV_EINVAL;
    if (*c->host_code) return UAVENV_EP2P;                     // sticky: this rank no longer steps (see the header comment)
    c->seq += 1;
    c->carry_cur = c->check_pending ? c->pending_idx : -1;
    hipLaunchKernelGGL(k_p2p_reduce_push, dim3((P + 4 + 31) / 32), dim3(256), 0, (hipStream_t)stream, partials, n_partials, P,
                       uavenv_dqn_partial_stride(net), dev_view(c, c->carry_cur, -1));
    if (hipGetLastError() != hipSuccess) {
        c->seq -= 1;                                           // nothing was enqueued: the sequence number is not used up
        return UAVENV_EHIP;
    }
    c->check_pending = false;
    return UAVENV_OK;
}

int uavenv_dqn_adam_p2p(const UavDqnNet *net, UavP2P *c, float lr, float beta1, float beta2, float eps, int32_t step_t,
                        int32_t hard_update, float *loss_out, float *raw_out, void *stream)
{
    return uavenv_dqn_adam_p2p_img(net, c, lr, beta1, beta2, eps, step_t, hard_update, loss_out, raw_out, nullptr, stream);
}

int uavenv_dqn_adam_p2p_img(const UavDqnNet *net, UavP2P *c, float lr, float beta1, float beta2, float eps, int32_t step_t,
                            int32_t hard_update, float *loss_out, float *raw_out, float *image_dev, void *stream)
{
    if (image_dev && (!net || net->w != uavq::kW || net->hid != uavq::kHid || (((uintptr_t)image_dev) & 15u) != 0)) return UAVENV_EINVAL;
    if (!net || !c || !c->connected || c->seq == 0) return UAVENV_EINVAL;
    const int P = uavenv_dqn_num_params(net);
    if (P <= 0 || P + 2 > c->bucket) return UAVENV_EINVAL;
    const bool apply = step_t > 0;                        // step_t == 0: only sum into raw_out (self-test)
    if (apply && (!net->local || !net->target || !net->m || !net->v)) return UAVENV_EINVAL;
    if (!apply && !raw_out) return UAVENV_EINVAL;
    const float bc1 = apply ? 1.0f - powf(beta1, (float)step_t) : 1.0f;
    const float bc2 = apply ? 1.0f - powf(beta2, (float)step_t) : 1.0f;
    const bool fold = apply && c->check_every > 0 && c->seq % c->check_every == 0;
    const int fold_idx = fold ? (int)(c->n_checks & 1u) : -1;
    hipLaunchKernelGGL(k_p2p_pull_adam, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, dev_view(c, c->carry_cur, fold_idx),
                       apply ? net->local : (float *)nullptr, net->target, net->m, net->v, raw_out, P, lr, beta1, beta2, eps,
                       bc1, sqrtf(bc2), hard_update, loss_out, apply ? image_dev : (float *)nullptr);
    if (hipGetLastError() != hipSuccess) return UAVENV_EHIP;
    if (fold) {
        c->check_pending = true;
        c->pending_idx = fold_idx;
        c->n_checks += 1;
    }
    return *c->host_code ? UAVENV_EP2P : UAVENV_OK;
}

int uavenv_p2p_check_blocks(UavP2P *c, const float *const *blocks_dev, const int32_t *n_floats, int32_t n_blocks, void *stream)
{
    if (!c || !c->connected || !blocks_dev || !n_floats || n_blocks <= 0 || n_blocks > UAVENV_P2P_CHECK_MAX_BLOCKS) return UAVENV_EINVAL;
    if (*c->host_code) return UAVENV_EP2P;
    HashBlocks h;
    int most = 0;
    for (int b = 0; b < UAVENV_P2P_CHECK_MAX_BLOCKS; ++b) { h.block[b] = nullptr; h.n_floats[b] = 0; }
    for (int b = 0; b < n_blocks; ++b) {
        if (!blocks_dev[b] || n_floats[b] <= 0) return UAVENV_EINVAL;
        h.block[b] = blocks_dev[b]; h.n_floats[b] = n_floats[b];
        most = n_floats[b] > most ? n_floats[b] : most;
    }
    h.n_blocks = n_blocks;
    hipStream_t s = (hipStream_t)stream;
    // wsum[0] is the accumulator (the DQN path's fold / carry pair is not used on a generic exchange: check_every = 0 there);
    // the four floats to push live behind the error words
    float *buf4 = reinterpret_cast<float *>(c->check_buf);
    int gx = (most + 256 * 8 - 1) / (256 * 8);
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    hipLaunchKernelGGL(k_p2p_hash_blocks, dim3(gx, n_blocks), dim3(256), 0, s, h, c->wsum);
    hipLaunchKernelGGL(k_p2p_hash_words, dim3(1), dim3(1), 0, s, c->wsum, buf4);
    if (hipGetLastError() != hipSuccess) return UAVENV_EHIP;
    c->seq += 1;
    hipLaunchKernelGGL(k_p2p_push, dim3(1), dim3(256), 0, s, buf4, 1, dev_view(c, -1, -1));
    if (hipGetLastError() != hipSuccess) { c->seq -= 1; return UAVENV_EHIP; }
    hipLaunchKernelGGL(k_p2p_pull_check, dim3(1), dim3(64), 0, s, dev_view(c, 0, -1));      // carry >= 0: compare the pairs
    if (hipGetLastError() != hipSuccess) return UAVENV_EHIP;
    c->n_checks += 1;
    return *c->host_code ? UAVENV_EP2P : UAVENV_OK;
}

int uavenv_p2p_allreduce(UavP2P *c, float *buf_dev, int64_t count, void *stream)
{
    if (!c || !c->connected || !buf_dev || count <= 0 || (count & 3) || count > (int64_t)c->bucket_pad ||
        (((uintptr_t)buf_dev) & 15u) != 0)
        return UAVENV_EINVAL;
    if (*c->host_code) return UAVENV_EP2P;                     // sticky (see the header comment)
    c->seq += 1;
    const int count4 = (int)(count / 4);
    hipLaunchKernelGGL(k_p2p_push, dim3((count4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, buf_dev, count4, dev_view(c, -1, -1));
    if (hipGetLastError() != hipSuccess) {
        c->seq -= 1;
        return UAVENV_EHIP;
    }
    // At most 32 workgroups: every workgroup of this launch sits on its CU until the peers' blocks have arrived, and a CU that
    // hosts one cannot take a 160 KB-LDS workgroup (the SAC phase kernels).  Two ranks sharing ONE device (the same-device test
    // runs) deadlocked on that until the wait timed out, about one run in eight: rank A's 340 waiting workgroups covered every CU
    // while rank B's gradient launch -- whose result A was waiting for -- could not be placed.  On a device of its own the cap
    // costs nothing: 87 k floats are three trips of 32 x 256 threads x 16 bytes.
    const int pull_wgs = (count4 + 255) / 256 < 32 ? (count4 + 255) / 256 : 32;
    hipLaunchKernelGGL(k_p2p_pull_sum, dim3(pull_wgs), dim3(256), 0, (hipStream_t)stream, dev_view(c, -1, -1), buf_dev, (int)count);
    if (hipGetLastError() != hipSuccess) return UAVENV_EHIP;
    return *c->host_code ? UAVENV_EP2P : UAVENV_OK;
}

}  // extern "C"
