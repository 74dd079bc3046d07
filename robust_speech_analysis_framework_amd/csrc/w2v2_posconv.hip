// Wav2Vec2 forward, positional stage: the grouped positional convolution (LDS-resident image, batched GEMM or exact fp32) and
// data2vec-audio's convolution stack; the kernels, then the Forward phases that launch them.
#include <type_traits>

#include "w2v2_forward.h"

namespace rsaf {
namespace w2v2 {

// ---- regroup for the grouped positional conv: xg[chunk][g][tt][ci], zero padded in time -----------
__global__ __launch_bounds__(256) void regroup_kernel(const float4* __restrict__ x, float4* __restrict__ xg, int n,
                                                      int T, int Hd4, int G, int K) {
    const int cg4 = Hd4 / G;
    const int TT = T + K - 1;
    const int64_t total = (int64_t)n * G * TT * cg4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i % cg4);
        int64_t r = i / cg4;
        const int tt = (int)(r % TT); r /= TT;
        const int g = (int)(r % G);
        const int64_t chunk = r / G;
        const int t = tt - K / 2;
        xg[i] = (t >= 0 && t < T) ? x[(chunk * T + t) * Hd4 + g * cg4 + ci] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the same regrouping as two fp16 planes (A operand of the positional convolution on the f16x3 GEMM), scaled per window by
// the power of two that the window's largest |x| (reported by the feature projection's epilogue) asks for
__global__ __launch_bounds__(256) void regroup_planes_kernel(const float4* __restrict__ x, unsigned short* __restrict__ xg,
                                                             int64_t plane, int n, int Tmax, int Hd4, int G, int K,
                                                             const int* __restrict__ Tw, const int64_t* __restrict__ row0,
                                                             const unsigned* __restrict__ amax, float* __restrict__ win_scale) {
    // destination per (window, group): Tmax + K - 1 rows of cg channels, frame t of window w at tt = t + K / 2, zeros around its T_w frames
    const int cg4 = Hd4 / G;
    const int TT = Tmax + K - 1;
    const int64_t total = (int64_t)n * G * TT * cg4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ci = (int)(i % cg4);
        int64_t r = i / cg4;
        const int tt = (int)(r % TT); r /= TT;
        const int g = (int)(r % G);
        const int64_t chunk = r / G;
        const int t = tt - K / 2;
        const float sc = f16x2_scale_for_bound(__uint_as_float(amax[chunk]));
        if (g == 0 && tt == 0 && ci == 0) win_scale[chunk] = sc;
        const float4 v = (t >= 0 && t < Tw[chunk]) ? x[(row0[chunk] + t) * Hd4 + g * cg4 + ci] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float vv[4] = {v.x * sc, v.y * sc, v.z * sc, v.w * sc};
        unsigned short hh[4], ll[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split2_w(vv[k], hh[k], ll[k]);
        // k16 panels per (window, group): [cg / 16][TT][16] - tap k of output frame t is panel row t + k, so the GEMM's DMA
        // moves 32 consecutive rows of a panel as one contiguous KiB (a_tap_panels = cg / 16)
        unsigned short* pp = xg + ((((chunk * G + g) * (cg4 / 4) + (ci >> 2)) * TT + tt) * 16 + (ci & 3) * 4);
        *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
        *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
    }
}

// ---- positional convolution: the window's panel image stays in LDS -----------------------------------------------------------
// As a batched GEMM (gemm_f16x3, 256 x 64 tiles) every k-tile of the 128-tap convolution re-reads its A tile from L2 although
// consecutive taps differ by ONE ROW: 6.3 MB of DMA per tile, 755 GB per 1 000 clips, 6.7 TB/s - the kernel sat on the L2 -> LDS
// path at 125 TFLOP/s-equivalent whatever the tile shape.  Here a workgroup owns one (window, group): the group's cg channels of
// the zero-padded window ([cg / 16 panels][T_w + PK - 1 rows][16], both fp16 planes: 120 KB at base geometry) are fetched ONCE,
// tap k of output row t is LDS row t + k, and only the weights stream (6 KB per step of two k16 units, four stages).  Eight
// waves x 64 rows; v_mfma_f32_16x16x32_f16 so that the 48 output channels are three full column tiles; the arithmetic is the
// GEMM's (a_l b_h + a_h b_l + a_h b_h, fp32 accumulation, power-of-two scales undone in the epilogue, bias, GELU).
// Rows and halves are stored with the GEMM's swizzle (16-byte half h of row r in slot h ^ ((r >> 3) & 1)): lanes r and r + 8 of a
// fragment read then hit different banks for any tap offset.
typedef _Float16 pc_f16x8 __attribute__((ext_vector_type(8)));
typedef float pc_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* pc_lds_ptr;
typedef const __attribute__((address_space(1))) void* pc_glb_ptr;

// SPLIT = 2 (windows of at most 256 frames - the 5 s windows of the extractor give 249): 256 rows per workgroup, waves 0-3 take
// the even steps and waves 4-7 the odd ones (split K; the halves meet through LDS in front of the epilogue), so that all eight
// waves have rows to work on and each weight step is read from LDS by four waves instead of eight.
template <int NT, int SPLIT>
__global__ __launch_bounds__(512, 1) void posconv_f16x3_kernel(const unsigned short* __restrict__ xg, int64_t a_plane,
                                                               const unsigned short* __restrict__ wp, int64_t b_plane, int Hd,
                                                               const float* __restrict__ a_scale, const float* __restrict__ b_scale,
                                                               const float* __restrict__ bias, const int* __restrict__ Tw,
                                                               const int64_t* __restrict__ row0, float* __restrict__ y, int G, int TT,
                                                               int PK, int rows_alloc) {
    extern __shared__ __attribute__((aligned(1024))) unsigned short pc_sm[];
    constexpr int cg = 16 * NT, B_SEG = cg * 16, B_INSTR = cg / 8, RGRPS = 8 / SPLIT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.x / G, g = blockIdx.x - w * G;
    const int a_panel = PosconvLds{NT, SPLIT, rows_alloc}.a_panel();      // elements per (plane, panel)
    unsigned short* sA = pc_sm;
    unsigned short* sB = pc_sm + PosconvLds::ring_at(NT, a_panel);
    // the window's image -> LDS: instruction ii = (plane, panel, block of 32 rows), 1 KiB each
    {
        const int blocks = rows_alloc / 32, total = 2 * NT * blocks;
        const int r_in = lane >> 1, slot = lane & 1;
        for (int ii = wave; ii < total; ii += 8) {
            const int pp = ii / blocks, rb = ii - pp * blocks;             // pp = plane * NT + panel
            const int pl = pp / NT, panel = pp - pl * NT;
            const int row = rb * 32 + r_in;
            const int srow = row < TT ? row : TT - 1;
            const int chunk = slot ^ ((row >> 3) & 1);
            const unsigned short* src = xg + pl * a_plane + ((((int64_t)w * G + g) * NT + panel) * TT + srow) * 16 + chunk * 8;
            __builtin_amdgcn_global_load_lds((pc_glb_ptr)src, (pc_lds_ptr)(sA + pp * a_panel + rb * 512), 16, 0, 0);
        }
    }
    // weights: step j = units 2 j, 2 j + 1 (a unit = 16 k of one tap); stage layout [unit in pair][plane][cg rows][16].
    // Iteration i = steps SPLIT i .. SPLIT i + SPLIT - 1, ring of four iterations.
    const int nit = PK * NT / 2 / SPLIT;
    int64_t boff = 0;
    if (wave < B_INSTR) {
        const int c = wave * 64 + lane;                                    // 16-byte chunk of the stage
        const int seg = c / (2 * cg), within = c - seg * (2 * cg);
        const int row = within >> 1, slot = within & 1;
        boff = (int64_t)(seg & 1) * b_plane + ((int64_t)(seg >> 1) * Hd + (g * cg + row)) * 16 + (slot ^ ((row >> 3) & 1)) * 8;
    }
    auto b_dma = [&](int i) {
        if (wave < B_INSTR) {
#pragma unroll
            for (int kh = 0; kh < SPLIT; ++kh)
                __builtin_amdgcn_global_load_lds((pc_glb_ptr)(wp + boff + (int64_t)(SPLIT * i + kh) * 2 * Hd * 16),
                                                 (pc_lds_ptr)(sB + PosconvLds::stage_at(NT, SPLIT, i & 3, kh) + wave * 512), 16, 0, 0);
        }
    };
    b_dma(0);
    if (nit > 1) b_dma(1);
    if (nit > 2) b_dma(2);
    pc_f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = pc_f32x4{0.f, 0.f, 0.f, 0.f};
    const int r16 = lane & 15, q = lane >> 4, hlf = q & 1, upair = q >> 1;
    const int khalf = wave / RGRPS, m_base = (wave - khalf * RGRPS) * 64;
    // fragments of a step: B from its stage of the ring, A from the resident image at the step's tap
    struct Frag { pc_f16x8 ah[4], al[4], bh[NT], bl[NT]; };
    auto fetch = [&](int i, Frag& F) {
        const int unit = 2 * (SPLIT * i + khalf) + upair;
        const int tap = unit / NT, panel = unit - tap * NT;
        const unsigned short* bst = sB + PosconvLds::stage_at(NT, SPLIT, i & 3, khalf) + upair * 2 * B_SEG;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int brow = 16 * nt + r16;
            const int off = brow * 16 + ((hlf ^ ((brow >> 3) & 1)) << 3);
            F.bh[nt] = *reinterpret_cast<const pc_f16x8*>(bst + off);
            F.bl[nt] = *reinterpret_cast<const pc_f16x8*>(bst + B_SEG + off);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = m_base + 16 * mt + r16 + tap;
            const int off = panel * a_panel + row * 16 + ((hlf ^ ((row >> 3) & 1)) << 3);
            F.ah[mt] = *reinterpret_cast<const pc_f16x8*>(sA + off);
            F.al[mt] = *reinterpret_cast<const pc_f16x8*>(sA + NT * a_panel + off);
        }
    };
    auto mfmas = [&](const Frag& F) {                                     // product by product: 4 NT independent accumulators
#pragma unroll                                                             // between two instructions on the same one
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.al[mt], F.bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.ah[mt], F.bl[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F.ah[mt], F.bh[nt], acc[mt][nt], 0, 0, 0);
    };
    // Software pipeline: at the top of iteration i the fragments of iteration i are in registers; the wave waits for its share
    // of iteration i + 1's weights (issued two iterations ago), the barrier publishes everybody's and frees the ring slot of
    // iteration i + 3 (read as fragments during iteration i - 2), the DMA of iteration i + 3 goes out, the fragments of
    // iteration i + 1 are requested and the 36 MFMAs of this iteration run while they arrive.
    Frag F0, F1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the image and the first three weight iterations
    __syncthreads();
    fetch(0, F0);
    auto step = [&](int i, const Frag& cur, Frag& nxt) {
        if (i >= 1) {
            if (i + 2 < nit) { if constexpr (SPLIT == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        if (i + 3 < nit) b_dma(i + 3);
        if (i + 1 < nit) fetch(i + 1, nxt);
        mfmas(cur);
    };
    for (int i = 0; i < nit; i += 2) {                                     // nit is even (launcher)
        step(i, F0, F1);
        step(i + 1, F1, F0);
    }
    if constexpr (SPLIT == 2) {                                            // the odd steps' sums join the even steps' through LDS
        __syncthreads();                                                   // (the image is dead)
        float* red = reinterpret_cast<float*>(pc_sm) + PosconvLds::exchange_at(NT, wave - khalf * RGRPS);
        if (khalf == 1) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) red[((mt * NT + nt) * 4 + v) * 64 + lane] = acc[mt][nt][v];
        }
        __syncthreads();
        if (khalf == 1) return;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[mt][nt][v] += red[((mt * NT + nt) * 4 + v) * 64 + lane];
    }
    // epilogue: D of the 16 x 16 tile: lane (q, r16), register v = row 4 q + v, column r16
    const int Tv = Tw[w];
    const int64_t r0 = row0[w];
    const float sa_inv = pow2_inverse(a_scale[w]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = g * cg + 16 * nt + r16;
        const float inv = sa_inv * pow2_inverse(b_scale[col]);
        const float bs = bias[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int v = 0; v < 4; v += 2) {
                const int m = m_base + 16 * mt + 4 * q + v;
                const gelu_f32x2 g2 = gelu_pair(gelu_f32x2{acc[mt][nt][v] * inv + bs, acc[mt][nt][v + 1] * inv + bs});
                if (m < Tv) y[(r0 + m) * Hd + col] = g2.x;
                if (m + 1 < Tv) y[(r0 + m + 1) * Hd + col] = g2.y;
            }
    }
}

// ---- positional convolution STACK (RSAF_W2V2_POS_CONV_STACK: data2vec-audio) ---------------------------------------------------
// D layers of p <- GELU(LN(conv(p))): grouped convolution of PK taps with bias, LayerNorm over all Hd channels of a frame
// without weight or bias (eps 1e-5), GELU.  The LayerNorm couples the groups of a frame, so a layer is two launches:
//   posstack_conv_kernel  one workgroup = PS_ROWS frames of one (window, group): the pre-LN values (+ bias) as fp32 rows
//   posstack_rows_kernel  one wave per frame: LayerNorm + GELU over the Hd channels, out as the fp16 plane pair the next
//                         layer's convolution multiplies (or, after the last layer, as fp32 rows for encoder.layer_norm)
// The planes are plain packed rows [rows][Hd]; the convolution zero-fills the frames outside [0, T_w) of ITS window while it
// copies its row tile (+ PK - 1 halo rows) into LDS, so no halo ever reads a neighbouring window's rows and a ragged call
// computes what the per-window calls compute.  From layer 1 on |p| <= sqrt(Hd - 1) (GELU of a normalised row), so the A
// planes' power-of-two scale is a constant of the geometry; layer 0 reads x under the window's scale (W.fp_amax).
// The convolution is the f16x3 arithmetic of posconv_f16x3_kernel (a_l b_h + a_h b_l + a_h b_h on v_mfma_f32_16x16x32_f16, fp32
// accumulation), with the same LDS image layout ([plane][cg / 16 panels][rows][16], 16-byte halves swizzled by (row >> 3) & 1)
// and the same weight panels; PK cg / 16 may be odd (19 x 3 = 57 units of 16 k): the last MFMA's upper half multiplies zeros.
// Four waves x 64 rows; a wave reads its weight fragments from global memory (panel layout: 512 contiguous bytes per 16 lanes),
// one step ahead of the MFMAs that consume them.

template <int NT>
__global__ __launch_bounds__(256) void posstack_conv_kernel(const unsigned short* __restrict__ ap, int64_t a_plane,
                                                            const unsigned short* __restrict__ wp, int64_t b_plane, int Hd,
                                                            const float* __restrict__ a_scale, float a_scale_const,
                                                            const float* __restrict__ b_scale, const float* __restrict__ bias,
                                                            const int* __restrict__ Tw, const int64_t* __restrict__ row0,
                                                            float* __restrict__ pre, int PK, int tiles, int rows_alloc) {
    extern __shared__ __attribute__((aligned(16))) unsigned short ps_sm[];
    constexpr int cg = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.x / tiles, tile = blockIdx.x - w * tiles, g = blockIdx.y;
    const int Tv = Tw[w], t0 = tile * PS_ROWS;
    if (t0 >= Tv) return;                                                  // the whole workgroup: a window shorter than the longest
    const int64_t r0 = row0[w];
    const PosstackLds lds{NT, rows_alloc};
    const int a_panel = lds.a_panel();
    // the tile's image: LDS row lr = frame t0 - PK / 2 + lr of THIS window, zeros outside [0, T_w)
    {
        constexpr int chunks = 2 * NT;                                     // 16-byte pieces of a row's cg channels
        const int total = 2 * rows_alloc * chunks;
        for (int i = tid; i < total; i += 256) {
            const int ch = i % chunks, r = i / chunks;
            const int pl = r / rows_alloc, lr = r - pl * rows_alloc;
            const int t = t0 - PK / 2 + lr;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (t >= 0 && t < Tv) v = *reinterpret_cast<const uint4*>(ap + pl * a_plane + (r0 + t) * Hd + g * cg + ch * 8);
            *reinterpret_cast<uint4*>(ps_sm + lds.panel(pl, ch >> 1) + lr * 16 + (((ch & 1) ^ ((lr >> 3) & 1)) << 3)) = v;
        }
    }
    __syncthreads();
    const int nunits = PK * NT, nsteps = (nunits + 1) / 2;                 // a unit = 16 k of one tap; a step = one MFMA depth of 32
    const int r16 = lane & 15, q = lane >> 4, hlf = q & 1, upair = q >> 1;
    const int m_base = wave * 64;
    pc_f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = pc_f32x4{0.f, 0.f, 0.f, 0.f};
    struct BFrag { pc_f16x8 h[NT], l[NT]; };
    const pc_f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    // this lane's unit of step j (the upper half of an odd count's last step has none: its weights read as zeros)
    auto fetch_b = [&](int j, BFrag& B) {
        const int unit = 2 * j + upair;
        const bool ok = unit < nunits;
        const unsigned short* src = wp + ((int64_t)(ok ? unit : 0) * Hd + g * cg + r16) * 16 + hlf * 8;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            B.h[nt] = ok ? *reinterpret_cast<const pc_f16x8*>(src + nt * 256) : zero8;
            B.l[nt] = ok ? *reinterpret_cast<const pc_f16x8*>(src + b_plane + nt * 256) : zero8;
        }
    };
    auto mfmas = [&](int j, const BFrag& B) {
        const int unit = 2 * j + upair;
        const int u = unit < nunits ? unit : 0;
        const int tap = u / NT, panel = u - tap * NT;
        pc_f16x8 ah[4], al[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = m_base + 16 * mt + r16 + tap;
            const int off = panel * a_panel + row * 16 + ((hlf ^ ((row >> 3) & 1)) << 3);
            ah[mt] = *reinterpret_cast<const pc_f16x8*>(ps_sm + off);
            al[mt] = *reinterpret_cast<const pc_f16x8*>(ps_sm + NT * a_panel + off);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mt], B.h[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], B.l[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], B.h[nt], acc[mt][nt], 0, 0, 0);
    };
    BFrag B0, B1;
    fetch_b(0, B0);
    for (int j = 0; j < nsteps; j += 2) {
        if (j + 1 < nsteps) fetch_b(j + 1, B1);
        mfmas(j, B0);
        if (j + 1 < nsteps) {
            if (j + 2 < nsteps) fetch_b(j + 2, B0);
            mfmas(j + 1, B1);
        }
    }
    // epilogue: lane (q, r16), register v = row 4 q + v, column r16 of a 16 x 16 tile: the pre-LN value, scales undone, + bias
    const float sa_inv = pow2_inverse(a_scale ? a_scale[w] : a_scale_const);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = g * cg + 16 * nt + r16;
        const float inv = sa_inv * pow2_inverse(b_scale[col]);
        const float bs = bias[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = t0 + m_base + 16 * mt + 4 * q + v;
                if (m < Tv) pre[(r0 + m) * Hd + col] = acc[mt][nt][v] * inv + bs;
            }
    }
}

// One wave per frame of D <= 1024 channels.  MODE 0: the row as it is (layer 0's input x) -> planes under its window's scale
// (from the largest |x| of the window, which also goes to win_scale).  MODE 1: LayerNorm without weight or bias (eps 1e-5)
// + GELU -> planes under the constant scale.  MODE 2: the same -> fp32 rows of `out` (which may be `src`: the wave holds the row).
template <int MODE>
__global__ __launch_bounds__(256) void posstack_rows_kernel(const float* src, int64_t rows, int D, const int* __restrict__ rowwin,
                                                            const unsigned* __restrict__ amax, float* __restrict__ win_scale,
                                                            float const_scale, unsigned short* __restrict__ planes, int64_t plane,
                                                            float* out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int D4 = D >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(src + row * D);
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < D4) { v[i] = x4[idx]; s += (v[i].x + v[i].y) + (v[i].z + v[i].w); }
    }
    float sc = const_scale;
    if constexpr (MODE == 0) {
        const int w = rowwin[row];
        sc = f16x2_scale_for_bound(__uint_as_float(amax[w]));
        if (lane == 0) win_scale[w] = sc;                                  // every row of the window writes the same value
    } else {
        const float mean = wave_sum(s) / D;
        float qq = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx < D4) {
                const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
                qq += (a * a + b * b) + (c * c + d * d);
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(qq) / D + 1e-5f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const gelu_f32x2 e0 = gelu_pair(gelu_f32x2{(v[i].x - mean) * rstd, (v[i].y - mean) * rstd});
            const gelu_f32x2 e1 = gelu_pair(gelu_f32x2{(v[i].z - mean) * rstd, (v[i].w - mean) * rstd});
            v[i] = make_float4(e0.x, e0.y, e1.x, e1.y);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = lane + 64 * i;
        if (idx >= D4) continue;
        if constexpr (MODE == 2) {
            reinterpret_cast<float4*>(out + row * D)[idx] = v[i];
        } else {
            const float yy[4] = {v[i].x * sc, v[i].y * sc, v[i].z * sc, v[i].w * sc};
            unsigned short hh[4], ll[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split2_w(yy[k], hh[k], ll[k]);
            unsigned short* pp = planes + row * D + 4 * idx;
            *reinterpret_cast<uint2*>(pp) = make_uint2(hh[0] | ((unsigned)hh[1] << 16), hh[2] | ((unsigned)hh[3] << 16));
            *reinterpret_cast<uint2*>(pp + plane) = make_uint2(ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16));
        }
    }
}

// the kernels' NT: a group's 16 NT channels as column tiles of 16 (group widths 16, 32, 48 and 64); f(integral_constant<NT>)
template <class F>
static int with_nt(int nt, F&& f) {
    switch (nt) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// 5. positional conv embedding (grouped, weight norm folded), GELU, then the first LayerNorm of the encoder: x = LN(x + pos),
//    or, stable layer norm, h = x + pos stays un-normalised (the residual stream) and layer 0's LN1(h) goes to the planes
int Forward::positional_conv() {
    if (posconv_on_f16x3(c)) {
        RSAF_TRY(posconv_regroup_planes());
        const bool pc_off = [] { const char* e = getenv("RSAF_W2V2_POSCONV_GEMM"); return e && e[0] == '1'; }();   // per call: the tests toggle it
        RSAF_TRY((!pc_off && regime.posconv) ? posconv_lds() : posconv_batched_gemm());
    } else {                                                 // group widths that are no multiple of 16 (test geometries)
        RSAF_TRY(conv_runs_fp32(x, Wt + L.posw, Wt + L.posb, ACT_GELU, "w2v2_posconv_gemm", "w2v2_regroup"));
    }
    if (pre_ln) return ln_to_qkv(x, ws + W.y, Wt + L.layers[0].ln1g, Wt + L.layers[0].ln1b, gate_rows(), 0, true, x);
    return ln_to_qkv(x, ws + W.y, Wt + L.elng, Wt + L.elnb, x, 0, true);
}
// 5 (POS_CONV_STACK). p_0 = x, p_{i+1} = GELU(LN(conv_i(p_i))), i = 0..D-1 (LN without weight or bias, eps 1e-5), then
//    x = LN(x + p_D) as above.  The pre-LN rows of every layer go through W.y, which ends up holding p_D; the planes
//    between the layers live in W.xg (rows x Hd elements per plane: no padding rows, the kernel pads per window)
int Forward::positional_conv_stack() {
    const int D = c.pos_depth(), cg = Hd / c.PG;
    {
        ProfScope prof("w2v2_posconv_stack", s, 2.0 * (double)D * rows * cg * (double)c.PK * cg * c.PG, (double)D * rows * Hd * 16.0);
        RSAF_TRY(posstack_on_mfma(c) ? posstack_mfma(D) : posstack_fp32(D));
    }
    return ln_to_qkv(x, ws + W.y, Wt + L.elng, Wt + L.elnb, x, 0, true);
}
template <int MODE>
int Forward::posstack_rows(const float* src, float* dst) {
    hipLaunchKernelGGL(posstack_rows_kernel<MODE>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, src, rows, Hd, rowwin,
                       bits_at(W.fp_amax), ws + W.pos_scale, f16x2_scale_for_bound(sqrtf((float)Hd)), planes_at(W.xg), rows * Hd, dst);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
template <int NT>
int Forward::posstack_conv_launch(int i) {
    const int cg = Hd / c.PG, tiles = (Tt + PS_ROWS - 1) / PS_ROWS;
    const PosstackLds lds = PosstackLds::make(cg, c.PK);
    RSAF_CHECK_ARG((int64_t)n * tiles <= 0x7fffffffLL, "too many row tiles");
    RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)posstack_conv_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.bytes()));
    hipLaunchKernelGGL((posstack_conv_kernel<NT>), dim3((unsigned)(n * tiles), (unsigned)c.PG), dim3(256), lds.bytes(), s,
                       reinterpret_cast<const unsigned short*>(planes_at(W.xg)), rows * Hd,
                       reinterpret_cast<const unsigned short*>(planes_at(i ? W.wp_stack[i - 1] : W.wp_pos)), (int64_t)Hd * c.PK * cg, Hd,
                       i ? nullptr : ws + W.pos_scale, f16x2_scale_for_bound(sqrtf((float)Hd)), ws + (i ? W.ws_stack[i - 1] : W.ws_pos),
                       Wt + (i ? L.stackb[i - 1] : L.posb), Tw + (int64_t)6 * n, row0, ws + W.y, c.PK, tiles, lds.rows_alloc);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
int Forward::posstack_mfma(int D) {
    RSAF_TRY(posstack_rows<0>(x, nullptr));
    for (int i = 0; i < D; ++i) {
        RSAF_TRY(with_nt(Hd / c.PG / 16, [&](auto nt) { return posstack_conv_launch<decltype(nt)::value>(i); }));
        RSAF_TRY(i + 1 < D ? posstack_rows<1>(ws + W.y, nullptr) : posstack_rows<2>(ws + W.y, ws + W.y));
    }
    return RSAF_OK;
}
// other group widths (test geometries): the exact-fp32 path below, rows normalised in place
int Forward::posstack_fp32(int D) {
    for (int i = 0; i < D; ++i) {
        RSAF_TRY(conv_runs_fp32(i ? ws + W.y : x, Wt + (i ? L.stackw[i - 1] : L.posw), Wt + (i ? L.stackb[i - 1] : L.posb), ACT_NONE,
                                "w2v2_posstack_gemm_f32", nullptr));
        RSAF_TRY(posstack_rows<2>(ws + W.y, ws + W.y));
    }
    return RSAF_OK;
}
// A grouped convolution on the exact-fp32 GEMM, W.y = act(conv(src) + bias): per run of equal windows the regroup and one
// launch of the family `gemm_family`.  regroup_family: the family the regroup is reported under (NULL: not on its own)
int Forward::conv_runs_fp32(const float* src, const float* w, const float* bias, int act, const char* gemm_family,
                            const char* regroup_family) {
    const int cg = Hd / c.PG;
    for (const auto& tg : R.tgroups) {
        const int nw = tg.second - tg.first, Tq = R.T6[tg.first], TTq = Tq + c.PK - 1;
        const int64_t r0 = R.row0[tg.first];
        const int64_t t4 = (int64_t)nw * TTq * (Hd / 4);
        auto regroup = [&] {
            hipLaunchKernelGGL(regroup_kernel, dim3((unsigned)std::min<int64_t>((t4 + 255) / 256, 4096)), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(src + r0 * Hd), reinterpret_cast<float4*>(ws + W.xg), nw, Tq, Hd / 4,
                               c.PG, c.PK);
        };
        if (regroup_family) { ProfScope prof(regroup_family, s, 0.0, (double)t4 * 32); regroup(); }
        else regroup();
        RSAF_CHECK_HIP(hipGetLastError());
        GemmParams p = gemm_params_plain(ws + W.xg, w, ws + W.y + r0 * Hd, Tq, cg, c.PK * cg, cg, (int64_t)c.PK * cg, Hd);
        p.nz = nw * c.PG; p.nz2 = c.PG;
        p.sA1 = (int64_t)c.PG * TTq * cg; p.sA2 = (int64_t)TTq * cg;
        p.sB1 = 0; p.sB2 = (int64_t)cg * c.PK * cg;
        p.sC1 = (int64_t)Tq * Hd; p.sC2 = cg;
        p.bias = bias; p.sBias2 = cg; p.act = act;
        RSAF_TRY(launch_gemm_f32(p, s, gemm_family));
    }
    return RSAF_OK;
}
// the regrouped sequence as k16 panels of T_w + PK - 1 rows per (window, group): tap k = one row down
int Forward::posconv_regroup_planes() {
    const int TT = Tt + c.PK - 1;
    const int64_t tot4 = (int64_t)n * TT * (Hd / 4);
    ProfScope prof("w2v2_regroup", s, 0.0, (double)tot4 * 32);
    hipLaunchKernelGGL(regroup_planes_kernel, dim3((unsigned)std::min<int64_t>((tot4 + 255) / 256, 4096)), dim3(256),
                       0, s, reinterpret_cast<const float4*>(ws + W.x), reinterpret_cast<unsigned short*>(planes_at(W.xg)),
                       (int64_t)n * TT * Hd, n, Tt, Hd / 4, c.PG, c.PK, Tw + (int64_t)6 * n, row0, bits_at(W.fp_amax), ws + W.pos_scale);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
template <int NT, int SP>
int Forward::posconv_lds_launch() {
    const int cg = Hd / c.PG, TT = Tt + c.PK - 1;
    const PosconvLds lds = PosconvLds::make(cg, c.PK, SP);
    RSAF_CHECK_HIP(hipFuncSetAttribute((const void*)posconv_f16x3_kernel<NT, SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.bytes()));
    hipLaunchKernelGGL((posconv_f16x3_kernel<NT, SP>), dim3((unsigned)(n * c.PG)), dim3(512), lds.bytes(), s,
                       reinterpret_cast<const unsigned short*>(planes_at(W.xg)), (int64_t)n * TT * Hd,
                       reinterpret_cast<const unsigned short*>(planes_at(W.wp_pos)), (int64_t)Hd * c.PK * cg, Hd,
                       ws + W.pos_scale, ws + W.ws_pos, Wt + L.posb, Tw + (int64_t)6 * n, row0, ws + W.y, c.PG, TT, c.PK, lds.rows_alloc);
    RSAF_CHECK_HIP(hipGetLastError());
    return RSAF_OK;
}
// the window's image stays in LDS (posconv_f16x3_kernel); RSAF_W2V2_POSCONV_GEMM=1: the batched GEMM below (A/B)
int Forward::posconv_lds() {
    const int cg = Hd / c.PG;
    ProfScope prof("w2v2_posconv_gemm", s, 2.0 * (double)rows * cg * (double)c.PK * cg * c.PG, 0.0);
    return with_nt(cg / 16, [&](auto nt) {
        return regime.posconv == 2 ? posconv_lds_launch<decltype(nt)::value, 2>() : posconv_lds_launch<decltype(nt)::value, 1>();
    });
}
// grouped conv as a two-level batched GEMM on the f16x3 kernel's 256 x 64 tile: batch (window, group), M = T_w rows,
// N = cg output channels, K = PK cg
int Forward::posconv_batched_gemm() {
    const int cg = Hd / c.PG, TT = Tt + c.PK - 1;
    GemmH3Params p{};
    p.A = planes_at(W.xg); p.a_plane = (int64_t)n * TT * Hd; p.lda = 16; p.sA = (int64_t)c.PG * TT * cg; p.sA2 = (int64_t)TT * cg;
    p.a_panel = 1; p.a_panel_rows = TT; p.a_tap_panels = cg / 16;
    p.a_scale = ws + W.pos_scale; p.a_scale_zs = 1; p.a_scale_ms = 0;
    p.B = planes_at(W.wp_pos); p.b_plane = (int64_t)Hd * c.PK * cg; p.ldb = 16; p.b_panel = 1; p.b_panel_rows = Hd; p.sB2 = (int64_t)cg * 16;
    p.b_scale = ws + W.ws_pos;
    p.C = ws + W.y; p.ldc = Hd; p.sC = 0; p.sC2 = cg;
    p.bias = Wt + L.posb; p.sBias2 = cg;
    p.M = Tt; p.ztab = ztab + (int64_t)6 * n * 2; p.N = cg; p.K = c.PK * cg; p.nz = n * c.PG; p.nz2 = c.PG; p.act = ACT_GELU; p.alpha = 1.0f;
    return launch_gemm_f16x3(p, s, "w2v2_posconv_gemm");
}

}  // namespace w2v2
}  // namespace rsaf
