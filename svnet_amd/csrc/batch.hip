// One training / evaluation batch assembled on the device from a device-resident pool of clouds: what the reference's loaders do per
// sample on the host (data.py:165-170 translate_pointcloud, :192-198 ModelNet40, :284-294 ShapeNetPart, :327-337 ScanObjectNN), its
// collate, the per-batch rotation (main_cls_dgcnn.py:168-178) and the permute to [B,3,N] (:179), as ONE launch into the fixed buffers
// of a TrainStep / ForwardStep.
//
// Everything a cloud receives is a pure function of (seed, epoch, g), g = the cloud's position in the epoch order (counter-based
// splitmix64, the derivation in svnet_amd/data.py's docstring - this file restates it, tests/loader_ref.py restates it independently):
//   cloud_key = sm(sm(sm(seed) ^ epoch) ^ g)
//   point order = ascending order of ((sm(cloud_key + p) >> 16) << 16) | p,  p = 0 .. S-1  (S = N: FIRST_SHUFFLED, S = P: SUBSET)
//   uniform j   = (sm(cloud_key + 2^32 + j) >> 40) * 2^-24,  j = 0..2 scales, 3..5 shifts, 6..8 rotation
// This file is compiled with -ffp-contract=off (Makefile): every product and sum below is its own correctly rounded fp32 operation,
// so the host can restate the coordinates bit for bit.
//
// Shape of the kernel: one workgroup per cloud.  The S keys (8 B each, padded with ~0 to a power of two) are written to LDS, sorted
// there by a bitonic network (one workgroup barrier per compare-exchange step), then the same workgroup gathers the first N rows of
// the order: 12-byte rows of the pool in, three coalesced channel planes out.
//
// Per-point attributes (normals, colours: `attr` [M,P,A] -> `attr_out` [B,A,N]) ride in the same launch, as a second instantiation of the
// same body (batch_assemble_kernel<true>): the thread that gathered pool point p into slot n reads p's row of A floats and writes one
// float into each of the A channel planes.  The first `attr_vectors` groups of three channels are direction vectors and follow the
// normal's rule of svnet_amd/data.py's docstring (divide by the scales, renormalise, rotate); the rest are copied bit for bit.  A pool
// without attributes launches batch_assemble_kernel<false>, in which none of this exists.
#include "pointset.h"

namespace {

constexpr int BATCH_THREADS = 1024;
constexpr int64_t BATCH_MAX_SORT = 8192;       // 8 B x 8192 keys = 64 KiB of LDS: the most a launch gets without an opt-in
// data.py:166-167: factors U(2/3, 3/2), offsets U(-0.2, 0.2); the bounds are the doubles below rounded once to fp32
constexpr float SCALE_LO = (float)(2.0 / 3.0), SCALE_SPAN = (float)(3.0 / 2.0 - 2.0 / 3.0);
constexpr float SHIFT_LO = (float)-0.2, SHIFT_SPAN = (float)0.4;

__host__ __device__ __forceinline__ uint64_t sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float uniform24(uint64_t cloud_key, int j) {
    return (float)(uint32_t)(sm64(cloud_key + (1ull << 32) + (uint64_t)j) >> 40) * 0x1p-24f;
}

static inline int64_t pow2_at_least(int64_t s) {
    int64_t p = 1;
    while (p < s) p <<= 1;
    return p;
}

struct BatchArgs {
    const float* data; const int64_t* label; const int64_t* seg; const int64_t* order;
    int64_t M, P, N, first, count;
    uint64_t seed, epoch;
    int select_mode, scale_shift, rotate;
    int64_t num_cat, S, Spad;
    float* x; int64_t* y; int64_t* seg_out; float* onehot; float* params;
};

struct BatchAttr {
    const float* attr; float* out;      // [M,P,A] -> [B,A,N]
    int A, vec3;                        // channels; 3 * attr_vectors: channels 0 .. vec3-1 are direction vectors
};

// ATTR = false never looks at `at` (the launch passes an empty one)
template <bool ATTR>
__global__ __launch_bounds__(BATCH_THREADS) void batch_assemble_kernel(const BatchArgs a, const BatchAttr at) {
    extern __shared__ __align__(16) unsigned char batch_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(batch_lds);
    const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    // a slot past the valid count repeats the batch's first cloud (same g: same points, same augmentation)
    const uint64_t g = (uint64_t)(a.first + (b < a.count ? b : 0));
    const int64_t m = a.order[g];
    const bool valid = m >= 0 && m < a.M;          // an order entry outside the pool: the slot is poisoned below, nothing is read
    const uint64_t cloud_key = sm64(sm64(sm64(a.seed) ^ a.epoch) ^ g);

    // ---- the cloud's 16 parameters (every thread computes the same values; thread 0 stores them)
    float sc[3] = {1.f, 1.f, 1.f}, sh[3] = {0.f, 0.f, 0.f}, R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (a.scale_shift) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            sc[j] = SCALE_LO + SCALE_SPAN * uniform24(cloud_key, j);
            sh[j] = SHIFT_LO + SHIFT_SPAN * uniform24(cloud_key, 3 + j);
        }
    }
    if (a.rotate == SVNET_BATCH_ROTATE_Z) {
        float s, c;
        sincospif(2.f * uniform24(cloud_key, 6), &s, &c);
        R[0] = c; R[1] = -s; R[3] = s; R[4] = c;
    } else if (a.rotate == SVNET_BATCH_ROTATE_SO3) {
        // a uniform unit quaternion from three uniforms (Shoemake 1992), then the matrix of train.rotate_clouds
        const float u1 = uniform24(cloud_key, 6);
        const float ra = sqrtf(1.f - u1), rb = sqrtf(u1);
        float s2, c2, s3, c3;
        sincospif(2.f * uniform24(cloud_key, 7), &s2, &c2);
        sincospif(2.f * uniform24(cloud_key, 8), &s3, &c3);
        const float w = rb * c3, i = ra * s2, j = ra * c2, k = rb * s3;
        R[0] = 1.f - 2.f * (j * j + k * k); R[1] = 2.f * (i * j - k * w);       R[2] = 2.f * (i * k + j * w);
        R[3] = 2.f * (i * j + k * w);       R[4] = 1.f - 2.f * (i * i + k * k); R[5] = 2.f * (j * k - i * w);
        R[6] = 2.f * (i * k - j * w);       R[7] = 2.f * (j * k + i * w);       R[8] = 1.f - 2.f * (i * i + j * j);
    }
    if (t == 0) {
        float* pr = a.params + (int64_t)b * 16;
        for (int j = 0; j < 3; ++j) { pr[j] = sc[j]; pr[3 + j] = sh[j]; }
        for (int j = 0; j < 9; ++j) pr[6 + j] = R[j];
        pr[15] = 0.f;
        a.y[b] = valid ? a.label[m] : -1;
    }
    if (a.onehot) {
        const int64_t lab = valid ? a.label[m] : -1;
        for (int64_t c = t; c < a.num_cat; c += T) a.onehot[(int64_t)b * a.num_cat + c] = c == lab ? 1.f : 0.f;
    }

    // ---- the point order: keys into LDS, bitonic sort
    const bool sorted = a.select_mode != SVNET_BATCH_FIRST_ORDERED;
    if (sorted) {
        const int S = (int)a.S, Spad = (int)a.Spad;
        for (int p = t; p < Spad; p += T)
            keys[p] = p < S ? (((sm64(cloud_key + (uint64_t)p) >> 16) << 16) | (uint64_t)p) : ~0ull;
        __syncthreads();
        for (int k = 2; k <= Spad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < (Spad >> 1); q += T) {
                    const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo | j;      // the q-th pair at distance j
                    const uint64_t ka = keys[lo], kb = keys[hi];
                    if ((ka > kb) == ((lo & k) == 0)) { keys[lo] = kb; keys[hi] = ka; }
                }
                __syncthreads();
            }
        }
    }

    // ---- gather + transform: pool rows in, channel planes out
    const int64_t N = a.N;
    float* xb = a.x + (int64_t)b * 3 * N;
    for (int64_t n = t; n < N; n += T) {
        const int64_t p = sorted ? (int64_t)(keys[n] & 0xFFFFull) : n;
        float v0 = SVNET_QNAN, v1 = SVNET_QNAN, v2 = SVNET_QNAN;
        int64_t sg = -1;
        if (valid) {
            const float* row = a.data + ((int64_t)m * a.P + p) * 3;
            v0 = row[0]; v1 = row[1]; v2 = row[2];
            if (a.scale_shift) {
                v0 = v0 * sc[0] + sh[0];
                v1 = v1 * sc[1] + sh[1];
                v2 = v2 * sc[2] + sh[2];
            }
            if (a.rotate != SVNET_BATCH_ROTATE_NONE) {
                const float r0 = (R[0] * v0 + R[1] * v1) + R[2] * v2;
                const float r1 = (R[3] * v0 + R[4] * v1) + R[5] * v2;
                const float r2 = (R[6] * v0 + R[7] * v1) + R[8] * v2;
                v0 = r0; v1 = r1; v2 = r2;
            }
            if (a.seg_out) sg = a.seg[(int64_t)m * a.P + p];
        }
        xb[n] = v0;
        xb[N + n] = v1;
        xb[2 * N + n] = v2;
        if (a.seg_out) a.seg_out[(int64_t)b * N + n] = sg;
        if (ATTR) {
            // the row of the same pool point: A floats in, one float into each of the A planes (each plane coalesced over n)
            const float* arow = at.attr + ((int64_t)m * a.P + p) * at.A;        // (followed only when valid)
            float* ob = at.out + (int64_t)b * at.A * N + n;
            int c = 0;
            for (; c < at.vec3; c += 3) {
                float q0 = SVNET_QNAN, q1 = SVNET_QNAN, q2 = SVNET_QNAN;
                if (valid) {
                    q0 = arow[c]; q1 = arow[c + 1]; q2 = arow[c + 2];
                    if (a.scale_shift) {
                        // a normal takes the inverse transpose of the linear part: S^-1, then back to unit length
                        q0 = q0 / sc[0]; q1 = q1 / sc[1]; q2 = q2 / sc[2];
                        const float l = sqrtf(sq_len(q0, q1, q2));
                        if (l > 0.f) { q0 = q0 / l; q1 = q1 / l; q2 = q2 / l; }
                    }
                    if (a.rotate != SVNET_BATCH_ROTATE_NONE) {
                        const float r0 = (R[0] * q0 + R[1] * q1) + R[2] * q2;
                        const float r1 = (R[3] * q0 + R[4] * q1) + R[5] * q2;
                        const float r2 = (R[6] * q0 + R[7] * q1) + R[8] * q2;
                        q0 = r0; q1 = r1; q2 = r2;
                    }
                }
                ob[(int64_t)c * N] = q0;
                ob[(int64_t)(c + 1) * N] = q1;
                ob[(int64_t)(c + 2) * N] = q2;
            }
#pragma unroll 4
            for (; c < at.A; ++c) ob[(int64_t)c * N] = valid ? arow[c] : SVNET_QNAN;
        }
    }
}


}  // namespace

extern "C" int svnet_batch_supported(int64_t P, int64_t N, int select_mode) {
    if (P < 1 || N < 1 || N > P) return 0;
    if (select_mode == SVNET_BATCH_FIRST_ORDERED) return 1;
    if (select_mode != SVNET_BATCH_FIRST_SHUFFLED && select_mode != SVNET_BATCH_SUBSET) return 0;
    const int64_t S = select_mode == SVNET_BATCH_SUBSET ? P : N;
    return S <= BATCH_MAX_SORT ? 1 : 0;
}

extern "C" int svnet_batch_assemble_f32(const svnet_batch_desc* d, void* stream) {
    SVNET_REQUIRE(d, SVNET_E_ARG, "svnet_batch_assemble_f32: null descriptor");
    SVNET_REQUIRE(d->data && d->label && d->order && d->x && d->y && d->params, SVNET_E_ARG,
                  "svnet_batch_assemble_f32: null data / label / order / x / y / params");
    SVNET_REQUIRE((d->seg_out == nullptr) || d->seg, SVNET_E_ARG, "svnet_batch_assemble_f32: seg_out without a pool seg (null)");
    SVNET_REQUIRE((d->onehot == nullptr) || d->num_cat >= 1, SVNET_E_ARG, "svnet_batch_assemble_f32: onehot with num_cat %lld < 1",
                  (long long)d->num_cat);
    SVNET_REQUIRE((d->attr_out == nullptr) || d->attr, SVNET_E_ARG, "svnet_batch_assemble_f32: attr_out without a pool attr (null)");
    SVNET_REQUIRE((d->attr == nullptr) || (d->A >= 1 && d->A <= SVNET_BATCH_MAX_ATTR), SVNET_E_ARG,
                  "svnet_batch_assemble_f32: attr with A %lld outside 1 .. %d", (long long)d->A, SVNET_BATCH_MAX_ATTR);
    SVNET_REQUIRE((d->attr == nullptr) || (d->attr_vectors >= 0 && d->attr_vectors <= d->A / 3), SVNET_E_ARG,
                  "svnet_batch_assemble_f32: attr_vectors %lld: 3 x it outside 0 .. A = %lld", (long long)d->attr_vectors, (long long)d->A);
    SVNET_REQUIRE(d->M >= 1 && d->P >= 1 && d->N >= 1 && d->B >= 1 && d->L >= 1, SVNET_E_ARG,
                  "svnet_batch_assemble_f32: M, P, N, B, L must be positive");
    SVNET_REQUIRE(d->N <= d->P, SVNET_E_ARG, "svnet_batch_assemble_f32: N %lld > P %lld", (long long)d->N, (long long)d->P);
    SVNET_REQUIRE(d->count >= 1 && d->count <= d->B, SVNET_E_ARG, "svnet_batch_assemble_f32: count %lld outside 1 .. B = %lld",
                  (long long)d->count, (long long)d->B);
    SVNET_REQUIRE(d->first >= 0 && d->first <= d->L - d->count, SVNET_E_ARG, "svnet_batch_assemble_f32: first %lld + count %lld > L %lld",
                  (long long)d->first, (long long)d->count, (long long)d->L);
    SVNET_REQUIRE(d->select_mode >= SVNET_BATCH_FIRST_SHUFFLED && d->select_mode <= SVNET_BATCH_FIRST_ORDERED, SVNET_E_ARG,
                  "svnet_batch_assemble_f32: select_mode %d", d->select_mode);
    SVNET_REQUIRE(d->rotate >= SVNET_BATCH_ROTATE_NONE && d->rotate <= SVNET_BATCH_ROTATE_SO3, SVNET_E_ARG,
                  "svnet_batch_assemble_f32: rotate %d", d->rotate);
    SVNET_REQUIRE(d->B <= 65535, SVNET_E_ARG, "svnet_batch_assemble_f32: B %lld > 65535", (long long)d->B);
    SVNET_REQUIRE(svnet_batch_supported(d->P, d->N, d->select_mode), SVNET_E_UNSUPPORTED,
                  "svnet_batch_assemble_f32: P %lld, N %lld, select_mode %d: more than %lld keys to sort (64 KiB of LDS)", (long long)d->P,
                  (long long)d->N, d->select_mode, (long long)BATCH_MAX_SORT);
    BatchArgs a;
    a.data = d->data; a.label = d->label; a.seg = d->seg; a.order = d->order;
    a.M = d->M; a.P = d->P; a.N = d->N; a.first = d->first; a.count = d->count;
    a.seed = (uint64_t)d->seed; a.epoch = (uint64_t)d->epoch;
    a.select_mode = d->select_mode; a.scale_shift = d->scale_shift ? 1 : 0; a.rotate = d->rotate;
    a.num_cat = d->onehot ? d->num_cat : 0;
    a.x = d->x; a.y = d->y; a.seg_out = d->seg_out; a.onehot = d->onehot; a.params = d->params;
    const bool sorted = d->select_mode != SVNET_BATCH_FIRST_ORDERED;
    a.S = !sorted ? 0 : d->select_mode == SVNET_BATCH_SUBSET ? d->P : d->N;
    a.Spad = sorted ? pow2_at_least(a.S < 2 ? 2 : a.S) : 0;
    // one thread per compare-exchange pair of the sort, and no fewer than the gather can use; whole waves
    int64_t threads = sorted ? a.Spad / 2 : d->N;
    if (threads < d->N) threads = d->N;
    threads = svnet_cdiv(threads, SVNET_WAVE) * SVNET_WAVE;
    if (threads > BATCH_THREADS) threads = BATCH_THREADS;
    const size_t lds = (size_t)a.Spad * sizeof(uint64_t);
    if (d->attr_out) {
        const BatchAttr at{d->attr, d->attr_out, (int)d->A, 3 * (int)d->attr_vectors};
        hipLaunchKernelGGL(batch_assemble_kernel<true>, dim3((unsigned)d->B), dim3((unsigned)threads), lds, (hipStream_t)stream, a, at);
    } else {
        hipLaunchKernelGGL(batch_assemble_kernel<false>, dim3((unsigned)d->B), dim3((unsigned)threads), lds, (hipStream_t)stream, a, BatchAttr{});
    }
    SVNET_CHECK_LAUNCH("batch_assemble_kernel");
    return SVNET_OK;
}
