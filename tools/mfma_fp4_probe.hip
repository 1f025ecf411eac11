// Probe of v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (E2M1) operands on gfx950, as the matcher would use it: 256-bit
// descriptors spread to +-1 nibbles (bit 0 -> +1.0 = 0x2, bit 1 -> -1.0 = 0xA), four K = 64 steps, unit scales (E8M0 127).
// Checks (i) exactness: D[row][col] = 256 - 2 Hamming(a_row, b_col) for random bits, (ii) the result layout
// col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), (iii) times a dependent-free stream of them, and
// (iv) the three ways of getting the matcher's key dot * 16384 - index out of the multiply instead of a v_fma_f32 per result
// (match.hip), each against the integer key for every index 0 .. 16383 at dot = -256, -2, 0, 2, 256:
//   form 1  block scales 2^7 x 2^7 on the four descriptor steps: the accumulator holds dot * 16384, the key needs one v_add_f32;
//   form 2  a fifth K-step: A = +1.0 nibbles, B = -index in E2M1 values (index & 127 as up to 32 values from {0 .. 6} at scale
//           2^0 in the positions the lower lanes carry, index >> 7 the same way at scale 2^7 in the upper lanes'), issued
//           behind the descriptor steps (2a) or in front of them (2b); and the pad code (all -6.0 at 2^17: finite and low);
//   form 3  -index as the C operand of the first descriptor step.
// Form 2 adds products of magnitude 0.5 .. 768 onto an accumulator near 2^22 inside one instruction: exact only if the
// hardware's internal alignment keeps the low bits.
// hipcc --offload-arch=gfx950 -O2 -o mfma_fp4_probe tools/mfma_fp4_probe.hip && ./mfma_fp4_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t spread8(uint32_t b) {   // 8 bits -> 8 nibbles 0x2 | bit << 3
    uint32_t x = (b | (b << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return (x << 3) | 0x22222222u;
}
__device__ __forceinline__ v8i operand(const uint32_t *desc, int step, int half) {   // bits [64 step + 32 half, + 32)
    const uint32_t w = desc[2 * step + half];
    v8i r = {(int)spread8(w & 0xFF), (int)spread8((w >> 8) & 0xFF), (int)spread8((w >> 16) & 0xFF), (int)spread8(w >> 24), 0, 0, 0, 0};
    return r;
}

__global__ void probe(const uint32_t *a, const uint32_t *b, float *out) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    v16f c = {0};
    for (int s = 0; s < 4; s++)
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(operand(a + 8 * r, s, h), operand(b + 8 * r, s, h), c, 4, 4, 0, 0x7F7F7F7F, 0,
                                                            0x7F7F7F7F);
    for (int g = 0; g < 16; g++) out[lane * 16 + g] = c[g];
}

// ---- (iv) keys.  One wave per tile of 32 train columns; row r has Hamming distance kHam[r % 5] to every column.
__device__ __forceinline__ v8i index_chunk(int v) {   // -v, 0 <= v <= 127, as 32 E2M1 nibbles: sixes, then the remainder
    uint32_t w[4] = {0, 0, 0, 0};
    int pos = 0;
    auto put = [&](uint32_t code) { w[pos >> 3] |= (code | 0x8u) << (4 * (pos & 7)); pos++; };
    for (; v >= 6; v -= 6) put(0x7);                       // 6.0
    const uint32_t code[6] = {0x0, 0x2, 0x4, 0x5, 0x6, 0x6};   // 0, 1, 2, 3, 4, (4 + 1)
    if (v) put(code[v]);
    if (v == 5) put(0x2);
    v8i r = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
    return r;
}
__global__ void keys(const uint32_t *base, int *bad) {   // bad[0..4]: form 1, 2a, 2b, 3, pad
    const int kHam[5] = {256, 129, 128, 127, 0};
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5, tile = blockIdx.x;
    uint32_t arow[8];
    for (int k = 0; k < 8; k++) arow[k] = base[k];
    for (int i = 0, p = (7 * r) & 255; i < kHam[r % 5]; i++, p = (p + 1) & 255) arow[p >> 5] ^= 1u << (p & 31);
    const int idx = tile * 32 + r;                          // the lane's train column
    const int s7 = 0x86868686, s0 = 0x7F7F7F7F;             // E8M0: 2^7, 2^0
    const v8i ones = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    const v8i bidx = index_chunk(h ? idx >> 7 : idx & 127);
    const int sidx = h ? 0x86868686 : s0;
    const v8i bpad = {h ? 0 : -1, h ? 0 : -1, h ? 0 : -1, h ? 0 : -1, 0, 0, 0, 0};
    const int spad = 0x90909090;                            // 2^17
    const float nidx = -(float)idx;
    v16f z = {0}, c1 = z, c2b, c3;
    for (int g = 0; g < 16; g++) c3[g] = nidx;
    c2b = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones, bidx, z, 4, 4, 0, s0, 0, sidx);
    for (int s = 0; s < 4; s++) {
        const v8i a = operand(arow, s, h), b = operand(base, s, h);
        c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c1, 4, 4, 0, s7, 0, s7);
        c2b = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c2b, 4, 4, 0, s7, 0, s7);
        c3 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c3, 4, 4, 0, s7, 0, s7);
    }
    const v16f c2a = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones, bidx, c1, 4, 4, 0, s0, 0, sidx);
    const v16f cp = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones, bpad, c1, 4, 4, 0, s0, 0, spad);
    for (int g = 0; g < 16; g++) {
        const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
        const float want = (float)((256 - 2 * kHam[row % 5]) * 16384 - idx);   // below 2^23: exact
        if (c1[g] + nidx != want) atomicAdd(&bad[0], 1);
        if (c2a[g] != want) atomicAdd(&bad[1], 1);
        if (c2b[g] != want) atomicAdd(&bad[2], 1);
        if (c3[g] != want) atomicAdd(&bad[3], 1);
        if (!(cp[g] < -4210688.f && cp[g] > -67108864.f)) atomicAdd(&bad[4], 1);   // below every real key, above "no candidate"
    }
}

__global__ void rate(const uint32_t *a, const uint32_t *b, float *out, int iters) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    v8i x[4], y[4];
    for (int s = 0; s < 4; s++) {
        x[s] = operand(a + 8 * r, s, h);
        y[s] = operand(b + 8 * r, s, h);
    }
    v16f c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
    for (int i = 0; i < iters; i++) {
        c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x[0], y[0], c0, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x[1], y[1], c1, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        c2 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x[2], y[2], c2, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        c3 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x[3], y[3], c3, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
}

int main() {
    std::vector<uint32_t> a(32 * 8), b(32 * 8);
    uint64_t s = 88172645463325252ull;
    auto rnd = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); };
    for (auto &v : a) v = rnd();
    for (auto &v : b) v = rnd();
    uint32_t *da, *db;
    float *dout;
    hipMalloc(&da, 1024); hipMalloc(&db, 1024); hipMalloc(&dout, 4 * 256 * 1024);
    hipMemcpy(da, a.data(), 1024, hipMemcpyHostToDevice);
    hipMemcpy(db, b.data(), 1024, hipMemcpyHostToDevice);
    probe<<<1, 64>>>(da, db, dout);
    std::vector<float> out(64 * 16);
    hipMemcpy(out.data(), dout, 64 * 16 * 4, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int lane = 0; lane < 64; lane++)
        for (int reg = 0; reg < 16; reg++) {
            const int col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            int ham = 0;
            for (int k = 0; k < 8; k++) ham += __builtin_popcount(a[row * 8 + k] ^ b[col * 8 + k]);
            const float want = (float)(256 - 2 * ham);
            if (out[lane * 16 + reg] != want) {
                if (bad < 8) printf("lane %d reg %d: got %g want %g\n", lane, reg, out[lane * 16 + reg], want);
                bad++;
            }
        }
    printf("mismatches: %d of 1024\n", bad);
    {   // (iv) 512 tiles x 32 columns = every index, 32 rows = the five dots six times over
        int *dbad, hbad[5];
        hipMalloc(&dbad, sizeof(hbad));
        hipMemset(dbad, 0, sizeof(hbad));
        keys<<<512, 64>>>(da, dbad);
        hipMemcpy(hbad, dbad, sizeof(hbad), hipMemcpyDeviceToHost);
        const char *name[5] = {"form 1 (scales 2^14, v_add)", "form 2a (index step last)", "form 2b (index step first)", "form 3 (index as C)",
                               "pad code (finite and low)"};
        for (int i = 0; i < 5; i++) printf("keys, %-28s: %d mismatches of %d\n", name[i], hbad[i], 512 * 64 * 16);
        for (int i = 0; i < 5; i++) bad += hbad[i];   // (match.hip's product kernel uses none of them: a record of what the hardware does)
    }
    // rate: 1024 workgroups x 4 waves, each 4 independent accumulators
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 4096;
    rate<<<1024, 256>>>(da, db, dout, 16);
    hipEventRecord(e0);
    rate<<<1024, 256>>>(da, db, dout, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    const double n = 1024.0 * 4 * iters * 4;                  // instructions
    printf("%.3f ms for %.0f MFMAs: %.1f cycles per instruction and SIMD at 2.4 GHz (4096 waves on 1024 SIMDs), %.2f Pop/s\n", ms, n,
           ms * 1e-3 * 2.4e9 / (n / 1024.0), n * 2.0 * 32 * 32 * 64 / (ms * 1e-3) / 1e15);
    return bad != 0;
}
