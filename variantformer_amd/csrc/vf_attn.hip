// vf_attn_varlen_fwd: variable-length multi-head attention forward for gfx950 (flash-style, online
// softmax, no S x S matrix in memory).  bf16 Q/K/V/O, fp32 scores / softmax / accumulation.
//
// Roofline: HBM/L2-bound for the short sequences of this model (seq2reg windows <= 200 tokens, gene
// stream <= 201: intensity ~ s/2 flop/B), MFMA-bound only for the long shared-K/V cross attention.
// Algorithmic bytes per (sequence, head) = 2*dh*(2*sq + 2*sk); flops = 4*sq*sk*dh.
//
// Work split: block = (sequence, head, q-tile), 256 threads = 4 waves, each wave owns QG groups of
// 16 queries.  K/V tiles of 64 keys are staged through LDS (two stages, register-prefetched while
// the previous tile is being consumed -- T14 issue-early / write-late).
//
// MFMA formulation (v_mfma_f32_16x16x32_bf16, lane = (r = lane&15, g = lane>>4)):
//   S^T[key][q]  = K . Q^T   A = K rows (ds_read_b128 from the swizzled K tile), B = Q (registers);
//                  the accumulator leaves lane (r,g) with keys 16*kt+4g+reg of QUERY r, so the
//                  softmax row reduction is in-lane plus two cross-lane steps (xor 16, xor 32).
//   O^T[d][q]   += V^T . P^T A = V^T gathered by ds_read_b64_tr_b16 from the row-major V tile,
//                  B = P^T straight from the score registers (bf16-packed).  The contraction index
//                  of one 32-key step is permuted (element j of lane group g <-> key 4g+j for j<4,
//                  16+4g+(j-4) for j>=4) identically on both operands, so no lane movement is needed.
// dh = 48 (the modulator's 1536/32) is padded to 64 only along the QK^T contraction (zero chunks in
// the K tile and zero Q fragments); PV uses exactly dh/16 output tiles.
//
// Head-dim classes (vf_attn_varlen_fwd_v3): every multiple of 8 up to 256 runs the kernels of the smallest class
// (32 / 48 / 64 / 96 / 128 / 192 / 256) that holds it, instantiated with PAD = true and told the true dh at run time
// (AttnParamsPad::dh): loads fetch dh / 8 chunks per row and leave zeros in the class's remaining Q / K / V columns, stores write
// the columns < dh.  The arithmetic is the class's: the result equals, bit for bit, a class-dh call on operands whose head
// columns were zero-padded.  The PAD = false instantiations (the five class head dims themselves) never read AttnParamsPad::dh.
#include <stdlib.h>
#include <type_traits>
#include "vf_common.h"

namespace {

constexpr int BKV = 64;

// K tile: one row per key, the head dimension padded to 64 (dh <= 64: 128-byte rows, 8 chunks of 16 bytes) or to 128
// (dh = 96 / 128: 256-byte rows, 16 chunks); the classes 192 / 256 keep their width (384- / 512-byte rows, 24 / 32 chunks).
// Chunk c of row `row` is stored at chunk c ^ swz(row), which makes the ds_read_b128 of a 16-lane group (rows r = 0..15,
// same logical chunk) hit 16 distinct 16-byte bank slots: 128- and 384-byte rows alternate between the two halves of the
// 256-byte bank row, so 8 XOR values suffice (they only touch the low 3 bits of c: c ^ swz stays inside the row); 256- and
// 512-byte rows all start on the same bank and need all 16.
template <int DH>
struct KLayout {
    static constexpr int ROW = DH <= 64 ? 128 : DH <= 128 ? 256 : DH * 2;
    static constexpr int TILE = BKV * ROW;
    static constexpr int KS = DH <= 64 ? 2 : DH / 32;            // 32-deep MFMA steps of the QK^T contraction
    static __device__ __forceinline__ int swz(int row) { return (ROW == 128 || ROW == 384) ? (row >> 1) & 7 : row & 15; }
};

template <int DH>
struct VLayout {
    // V row stride in bytes: a multiple of 32 with an odd 32-byte count, so that the 8 rows a
    // 32-lane half touches in one transposed read fall on 8 distinct 32-byte bank windows.
    static constexpr int ROW = (((DH * 2) / 32) & 1) ? DH * 2 : DH * 2 + 32;
    static constexpr int TILE = BKV * ROW;
};

// For dh < 64 the QK^T contraction is padded to 64, so key masking rides on the MFMA: Q carries 1.0 in pad slot
// d = dh, K carries 0 (valid key) or -32768 (row past the sequence end) there.  Valid scores get exactly +0.0, masked
// scores ~ -7e3 after scaling -> exp2 underflows to 0.  dh = 64 has no spare slot and masks on the VALU.
template <int DH> struct HwMask { static constexpr bool value = DH < 64; };
template <int DT> __device__ __forceinline__ u32x4_t mask_chunk(bool valid) { return (u32x4_t){valid ? 0u : Op16<DT>::NEG_BIG, 0u, 0u, 0u}; }
template <int DT> __device__ __forceinline__ u32x4_t q_pad_chunk(int d0, int dh) { return (u32x4_t){d0 == dh ? Op16<DT>::ONE : 0u, 0u, 0u, 0u}; }

// max over the lanes {l, l^16, l^32, l^48} (the four key sub-blocks g of one query) without LDS round trips:
// v_permlane16_swap / v_permlane32_swap exchange 16- / 32-lane rows on the VALU (lane semantics checked by
// tools/hw_probe.hip), replacing two ds_bpermute on the serial softmax chain.
// max(a, b, c): hipcc selects ONE v_max3_f32 for this shape (the file is built with -fno-honor-nans, so no
// canonicalising v_max_f32 x, x is put in front of it).  NOT inline asm: the hazard recognizer does not see inside an
// asm statement, and an MFMA result needs software wait states before a VALU instruction may read it.
__device__ __forceinline__ float max3f(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float max2f(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ float max_over_g(float x) {
    const unsigned u = __float_as_uint(x);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float y = max2f(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned v = __float_as_uint(y);
    auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return max2f(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

struct AttnParams {
    const unsigned short* q;
    const unsigned short* k;
    const unsigned short* v;
    unsigned short* out;
    int64_t q_stride, k_stride, v_stride, o_stride;
    const int32_t* cu_q;
    const int32_t* cu_k;
    const float* slopes;
    float scale_log2;   // scale * log2(e)
    int H;
    int nqb;            // query blocks per (sequence, head) (tiled kernel)
    int chunk;          // blocks per XCD = ceil(n_seq * H * nqb / 8)
    int total;          // n_seq * H * nqb
    int q_at_start;     // ALiBi query positions: 0 = queries are the LAST len_q positions of the key sequence
                        // (flash-attn convention), 1 = query i sits at position i
    int q_log2;         // 1: Q was projected with weights pre-multiplied by scale * log2(e) (VF_ATTN_Q_LOG2): scores are
                        // base-2 logits as they leave the matrix pipe, scale_log2 = 1
    const int64_t* q_rows;   // optional row maps (vf_attn_varlen_fwd_rows): token t's query row is row q_rows[t] of q, its key /
    const int64_t* kv_rows;  // value rows are row kv_rows[t] of k / v -- the operands are TABLES of distinct rows (the first
                             // layers' projections by lookup) and the gather happens in the loads; null: row t itself
};

// The padded-class kernels' argument (PAD = true): AttnParams plus the true head dim, a multiple of 8 below the class DH.  A
// type of its own, so that the arguments -- and the code -- of the class instantiations stay exactly what they were.
struct AttnParamsPad : AttnParams {
    int dh;
};
template <bool PAD> using AttnArgs = typename std::conditional<PAD, AttnParamsPad, AttnParams>::type;
// the kernels' `const int dh = PAD ? pad_dh(P) : DH;` is a constant expression in the class instantiations
__device__ __forceinline__ int pad_dh(const AttnParamsPad& P) { return P.dh; }
__device__ __forceinline__ int pad_dh(const AttnParams&) { return 0; }

// Block -> (sequence, head, query block).  Workgroups are dealt to the 8 XCDs round-robin by linear id, so XCD x gets
// the logical range [x * chunk, (x + 1) * chunk): all heads and query blocks of a sequence run on one XCD at about the
// same time.  Their K/V re-reads and the cache lines that neighbouring heads share then hit that XCD's L2, and the
// 96/128-byte head slices of one token row reach HBM together instead of one DRAM page activation per slice.
// Logical order: query block fastest, then head, then sequence.  Returns false for the padding blocks.
__device__ __forceinline__ bool block_coords(const AttnParams& P, int& seq, int& h, int& qb) {
    const int id = blockIdx.x;
    const int L = (id & 7) * P.chunk + (id >> 3);
    if ((id >> 3) >= P.chunk || L >= P.total) return false;
    qb = L % P.nqb;
    const int sh = L / P.nqb;
    h = sh % P.H;
    seq = sh / P.H;
    return true;
}

// out[tok0 .. tok0+n)[head h] = 0 (sequences without keys)
template <int DH, bool PAD = false>
__device__ __forceinline__ void zero_rows(const AttnArgs<PAD>& P, int tok0, int n, int h) {
    const int dh = PAD ? pad_dh(P) : DH;
    const int CPR = dh / 4;                           // 8-byte pieces (the output is only 8-byte aligned)
    for (int i = threadIdx.x; i < n * CPR; i += blockDim.x)
        *reinterpret_cast<u32x2_t*>(P.out + (int64_t)(tok0 + i / CPR) * P.o_stride + h * dh + (i % CPR) * 4) =
            (u32x2_t){0u, 0u};
}

__device__ __forceinline__ s16x4_t lds_tr_read(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}

// One 64-key tile for QG query groups of a wave: S^T = K.Q^T, online softmax, O^T += V^T.P^T.
// sK / sV point at the tile's first key row in LDS.  All state is per lane (r = query, g = key sub-block).
// NKT (4, 2 or 1): number of 16-key sub-tiles that can hold a valid key -- the LAST tile of a sequence whose remainder is
// <= 32 / <= 16 keys runs the 2 / 1 sub-tile form: no K fragments, QK^T MFMAs, bias, maximum, exponentials for the rest, and
// for NKT <= 2 no second 32-key PV block either.  Bit-identical to the full tile (whose masked keys contribute p = 0 exactly,
// and x + 0 = x in the accumulators); a 201-key sequence (3 tiles + 9 keys) saves 3/16 of its arithmetic.
// SM (softmax mode): 0 = online softmax with a running maximum, scale applied here; 1 and 2: q carries the base-2 softmax
// scale (AttnParams::q_log2) -- 1 = NO maximum: p = exp2(s [+ bias]), unnormalised sums; the caller checks the denominators
// and recomputes with mode 2 when one left the safe range (see attn_x32_kernel); 2 = running maximum rounded up to an
// INTEGER: a power-of-two offset does not move the rounding of p, so modes 1 and 2 produce the same bits -- which is what
// lets the kernels a query may be served by differ in mode (a gene's result must not depend on the batch geometry that picks
// the kernel: the tiled kernels run mode 2, the one-block-per-sequence kernel mode 1).
template <int DH, int QG, bool ALIBI, int DT, int NKT = 4, int SM = 0>
__device__ __forceinline__ void attn_tile(const char* sK, const char* sV, int kb0, int len_k, int r, int g, float c,
                                          float slope2, const typename Op16<DT>::frag (&qf)[QG][KLayout<DH>::KS], const float (&q_pos)[QG],
                                          f32x4_t (&o)[QG][DH / 16], float (&m_run)[QG], f32x4_t (&l_acc)[QG]) {
    using frag_t = typename Op16<DT>::frag;
    constexpr int NDT = DH / 16;
    constexpr int VROW = VLayout<DH>::ROW;
    constexpr int KS = KLayout<DH>::KS, K_ROW_BYTES = KLayout<DH>::ROW;
    // ---- S^T = K . Q^T : 4 key tiles x 2 k-steps, K fragments shared by the QG query groups
    f32x4_t s[QG][4];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) s[qg][kt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // all 8 K fragments of the tile are requested before the first MFMA and the V fragments of the first 32-key
    // block right after, so LDS latency overlaps the MFMAs and the softmax arithmetic instead of preceding every
    // MFMA pair (diagnostic builds: just-in-time fragment reads cost ~70 of 150 us on the gene->CRE shape)
    frag_t kf[NKT][KS];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            kf[kt][ks] = *reinterpret_cast<const frag_t*>(
                sK + (16 * kt + r) * K_ROW_BYTES + (((4 * ks + g) ^ KLayout<DH>::swz(r)) << 4));
    auto read_v = [&](int kb, frag_t(&vf)[NDT]) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const char* vp = sV + (32 * kb + 4 * g + (r >> 2)) * VROW + 32 * dt + 8 * (r & 3);
            const s16x4_t lo = lds_tr_read(vp);
            const s16x4_t hi = lds_tr_read(vp + 16 * VROW);
            vf[dt] = __builtin_bit_cast(frag_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
    };
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int qg = 0; qg < QG; ++qg)
                s[qg][kt] = Op16<DT>::mfma(kf[kt][ks], qf[qg][ks], s[qg][kt]);
    frag_t vf0[NDT];
    read_v(0, vf0);

    // ---- online softmax (lane (r,g): query r, keys kb0 + 16kt + 4g + e), in three steps so that the long part is
    // ONE basic block in which matrix and vector instructions can be interleaved:
    //   (1) bias / mask and the running maximum of every query group;
    //   (2) ONE wave-uniform branch: rescale O and l of all groups when any running maximum moved (alpha is exactly 1
    //       for the rows whose maximum did not move, so the result is the same as a per-group test);
    //   (3) per group: p = exp2(...), pack to 16 bit -- followed in program order by the PV / row-sum MFMAs of the
    //       PREVIOUS group, which have no dependence on this group's exponentials: the wave issues in order, so this
    //       is what lets the matrix pipe work under the v_exp stream (before: 250 VALU instructions with an idle
    //       matrix pipe, then 21 MFMAs back to back with an idle VALU).
    frag_t pf[QG][2];
    const bool tail = kb0 + BKV > len_k;           // wave-uniform: only the last (ragged) key tile masks keys
    const int klim = len_k - kb0 - 4 * g;          // key 16kt+e of this lane is valid iff 16kt+e < klim
    const float k_pos0 = (float)(kb0 + 4 * g);
    constexpr unsigned int one2 = Op16<DT>::ONE * 0x10001u;
    const u32x4_t ones_bits = {one2, one2, one2, one2};
    const frag_t ones = __builtin_bit_cast(frag_t, ones_bits);
    auto pack_p = [&](int qg) {                        // sub-tiles kt >= NKT still hold their initial zeros = 16-bit zeros
#pragma unroll
        for (int kb = 0; kb < (NKT > 2 ? 2 : 1); ++kb) {
            u32x4_t pk;
            pk[0] = Op16<DT>::pack2(s[qg][2 * kb][0], s[qg][2 * kb][1]);
            pk[1] = Op16<DT>::pack2(s[qg][2 * kb][2], s[qg][2 * kb][3]);
            pk[2] = Op16<DT>::pack2(s[qg][2 * kb + 1][0], s[qg][2 * kb + 1][1]);
            pk[3] = Op16<DT>::pack2(s[qg][2 * kb + 1][2], s[qg][2 * kb + 1][3]);
            pf[qg][kb] = *reinterpret_cast<frag_t*>(&pk);
        }
    };
    // O^T += V^T . P^T and the softmax denominators of one query group.  The denominators run on the matrix pipe: a
    // V^T fragment of ones gives l[q] += sum_k P[q][k] in every accumulator row, i.e. each lane ends up with the
    // complete row sum of its query (no per-element v_add_f32 -- the softmax is VALU-issue bound -- and no cross-lane
    // reduction at the end).  The sum runs over the 16-bit P the PV product uses, so O / l is an exact convex
    // combination of the V rows.
    frag_t vf1[NDT];
    auto pv = [&](int qg) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[qg][dt] = Op16<DT>::mfma(vf0[dt], pf[qg][0], o[qg][dt]);
        if (NKT > 2) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[qg][dt] = Op16<DT>::mfma(vf1[dt], pf[qg][1], o[qg][dt]);
        }
        l_acc[qg] = Op16<DT>::mfma(ones, pf[qg][0], l_acc[qg]);
        if (NKT > 2) l_acc[qg] = Op16<DT>::mfma(ones, pf[qg][1], l_acc[qg]);
    };
    float m_new[QG];
    bool moved = false;
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        if (ALIBI) {
            const float dq = q_pos[qg] - k_pos0;
            // q carries the scale (modes 1, 2, imax): bias and logit meet in ONE fused multiply-add, the same expression in
            // every kernel; otherwise scale and bias are applied together (wave-uniform choice)
            if (SM != 0) {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        s[qg][kt][e] = fmaf(-slope2, fabsf(dq - (float)(16 * kt + e)), s[qg][kt][e]);
            } else {
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        s[qg][kt][e] = fmaf(s[qg][kt][e], c, -slope2 * fabsf(dq - (float)(16 * kt + e)));
            }
        }
        if (tail && !HwMask<DH>::value) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[qg][kt][e] = (16 * kt + e) < klim ? s[qg][kt][e] : -INFINITY;
        }
        // 16 scores -> 1 maximum in 8 v_max3_f32 + 1 v_max_f32 (two chains of max(max(a, b), c) for instruction-level
        // parallelism; a pairwise tree compiled to 24 v_max / v_max3 per query group: the loop is VALU-issue bound)
        if (SM == 1) continue;
        float mxa = max3f(s[qg][0][0], s[qg][0][1], s[qg][0][2]), mxb;
        if (NKT == 4) {
            mxb = max3f(s[qg][2][0], s[qg][2][1], s[qg][2][2]);
            mxa = max3f(mxa, s[qg][0][3], s[qg][1][0]);
            mxb = max3f(mxb, s[qg][2][3], s[qg][3][0]);
            mxa = max3f(mxa, s[qg][1][1], s[qg][1][2]);
            mxb = max3f(mxb, s[qg][3][1], s[qg][3][2]);
            mxa = max3f(mxa, s[qg][1][3], s[qg][3][3]);
        } else if (NKT == 2) {
            mxb = max3f(s[qg][1][0], s[qg][1][1], s[qg][1][2]);
            mxa = max3f(mxa, s[qg][0][3], s[qg][1][3]);
        } else {
            mxb = s[qg][0][3];
        }
        float mx = max_over_g(max2f(mxa, mxb));
        if (SM == 2) mx = __builtin_ceilf(mx);
        m_new[qg] = max2f(m_run[qg], mx);           // finite: tile 0 always holds a valid key
        moved = moved || (m_new[qg] > m_run[qg]);
    }
    if (SM != 1 && __any(moved)) {                   // wave-uniform; rare after the first tiles of a sequence
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            const float alpha = __builtin_amdgcn_exp2f(ALIBI ? (m_run[qg] - m_new[qg]) : (m_run[qg] - m_new[qg]) * c);
            l_acc[qg] *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[qg][dt] *= alpha;
        }
    }
    if (NKT > 2) read_v(1, vf1);
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        if (SM == 1) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[qg][kt][e] = __builtin_amdgcn_exp2f(s[qg][kt][e]);
        } else {
            m_run[qg] = m_new[qg];
            // p = exp2(c*s - c*m) (no ALiBi: scale folded into one FMA) or exp2(s - m) (ALiBi: already scaled)
            const float mc = ALIBI ? -m_new[qg] : -m_new[qg] * c;
            const float cc = ALIBI ? 1.0f : c;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[qg][kt][e] = __builtin_amdgcn_exp2f(fmaf(s[qg][kt][e], cc, mc));
        }
        pack_p(qg);
        if (qg > 0) pv(qg - 1);
    }
    pv(QG - 1);
}

// The last key tile of a sequence in its short form: `rem` = keys it holds, <= 32 (the caller's tile loop stops one tile
// early for such a remainder; a longer one is an ordinary full tile of that loop -- no second copy of the full tile body).
template <int DH, int QG, bool ALIBI, int DT, int SM = 0>
__device__ __forceinline__ void attn_tile_short(int rem, const char* sK, const char* sV, int kb0, int len_k, int r, int g, float c,
                                                float slope2, const typename Op16<DT>::frag (&qf)[QG][KLayout<DH>::KS],
                                                const float (&q_pos)[QG], f32x4_t (&o)[QG][DH / 16], float (&m_run)[QG],
                                                f32x4_t (&l_acc)[QG]) {
    if (rem <= 16) attn_tile<DH, QG, ALIBI, DT, 1, SM>(sK, sV, kb0, len_k, r, g, c, slope2, qf, q_pos, o, m_run, l_acc);
    else attn_tile<DH, QG, ALIBI, DT, 2, SM>(sK, sV, kb0, len_k, r, g, c, slope2, qf, q_pos, o, m_run, l_acc);
}

// (2 query groups with ALiBi sit at the 170-register edge of three waves per SIMD -- the CRE stream's self attention; the
// integer-maximum form compiles to 172 without the bound)
// PAD: a head dim below the class DH (AttnParamsPad::dh, see the file header); classes 192 / 256 exist only in this form.
template <int DH, int QG, bool ALIBI, int DT = VF_BF16, bool QL = false, bool PAD = false>
__global__ __launch_bounds__(256, (QL && QG == 2 && ALIBI && DH <= 48 ? 3 : 1)) void attn_fwd_kernel(AttnArgs<PAD> P) {
    using frag_t = typename Op16<DT>::frag;
    const int dh = PAD ? pad_dh(P) : DH;               // true head dim: chunks [dh / 8, CPR) of a row are zeros in LDS
    constexpr int CPR = DH / 8;                       // 16-byte chunks per K/V row
    constexpr int NCHUNK = BKV * CPR;                 // chunks per tile
    constexpr int NLD = (NCHUNK + 255) / 256;         // chunk loads per thread per operand
    constexpr int NDT = DH / 16;                       // output d-tiles
    constexpr int VROW = VLayout<DH>::ROW;
    constexpr int KS = KLayout<DH>::KS, K_ROW_BYTES = KLayout<DH>::ROW, K_TILE_BYTES = KLayout<DH>::TILE;
    constexpr int STAGE = K_TILE_BYTES + VLayout<DH>::TILE;
    constexpr int BQ = 4 * QG * 16;

    extern __shared__ __attribute__((aligned(16))) char smem[];       // 2 * STAGE bytes (attn_fwd_lds<DH>())

    int seq, h, qblk;
    if (!block_coords(P, seq, h, qblk)) return;
    const int q_tok0 = P.cu_q[seq], len_q = P.cu_q[seq + 1] - q_tok0;
    const int k_tok0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k_tok0;
    const int qb0 = qblk * BQ;
    if (qb0 >= len_q) return;                         // block-uniform
    if (len_k <= 0) {                                 // no keys: the output rows are zeros (flash-attn convention)
        zero_rows<DH, PAD>(P, q_tok0 + qb0, (len_q - qb0) < BQ ? (len_q - qb0) : BQ, h);
        return;
    }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;

    // ---- zero the K pad chunks (d >= DH) of both stages once; loads never touch them
    // (chunk CPR is the mask slot and belongs to write_lds alone: zeroing it here as well would race with the mask
    // write of tile 0, which is issued by another wave without a barrier in between)
    if (CPR < 7) {                                    // dh = 32 / 48 only (dh >= 64 has no pad chunks that are read)
        constexpr int PADC = 7 - CPR;
        for (int i = tid; i < 2 * BKV * PADC; i += 256) {
            const int st = i / (BKV * PADC), rem = i % (BKV * PADC);
            const int row = rem / PADC, c = CPR + 1 + rem % PADC;
            *reinterpret_cast<u32x4_t*>(smem + st * STAGE + row * K_ROW_BYTES + ((c ^ ((row >> 1) & 7)) << 4)) =
                (u32x4_t){0u, 0u, 0u, 0u};
        }
    }

    // ---- Q fragments (B operand): lane (r,g) holds Q[q = r][d = 32ks + 8g .. +7]
    frag_t qf[QG][KS];
    int q_abs[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        q_abs[qg] = qb0 + (wave * QG + qg) * 16 + r;
        const int row = q_abs[qg] < len_q ? q_abs[qg] : len_q - 1;
        const unsigned short* qp = P.q + (int64_t)(q_tok0 + row) * P.q_stride + h * dh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int d0 = 32 * ks + 8 * g;
            u32x4_t raw = q_pad_chunk<DT>(d0, DH);
            if (d0 < dh) raw = *reinterpret_cast<const u32x4_t*>(qp + d0);
            qf[qg][ks] = *reinterpret_cast<frag_t*>(&raw);
        }
    }

    // scores live in the log2 domain: p = exp2(c*s + bias - m).  Without ALiBi the running max is kept on the RAW
    // score (c > 0, so the arg-max is the same) and scale and max are folded into one FMA per element.
    const float c = P.scale_log2;
    const float slope2 = ALIBI ? P.slopes[h] * 1.4426950408889634f : 0.f;
    float q_pos[QG];                                   // query position + (sk - sq), as float (exact: < 2^24)
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) q_pos[qg] = (float)(q_abs[qg] + (P.q_at_start ? 0 : len_k - len_q));

    f32x4_t o[QG][NDT];
    float m_run[QG];
    f32x4_t l_acc[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        m_run[qg] = -INFINITY;
        l_acc[qg] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[qg][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }

    // ---- K/V tile staging: global -> registers -> LDS.  The tile's K chunks and V chunks form ONE list of 2*NCHUNK
    // 16-byte items, exactly NLD2 per thread, so the prefetch has no divergent branch (with per-thread `if`s hipcc's
    // wait insertion drained the prefetch -- s_waitcnt vmcnt(0) -- in front of the first MFMA of every tile).
    constexpr int NLD2 = 2 * NCHUNK / 256;
    static_assert(2 * NCHUNK % 256 == 0, "staging items must divide over the threads");
    u32x4_t kvreg[NLD2];
    const unsigned short* kbase = P.k + (int64_t)k_tok0 * P.k_stride + h * dh;
    const unsigned short* vbase = P.v + (int64_t)k_tok0 * P.v_stride + h * dh;
    // per-item constants of the staging list: source pointer at key 0 of the sequence and the row stride; the per-tile
    // address is base + min(key, len_k - 1) * stride with a 24-bit multiply (full rate; max_seqlen_k * stride < 2^31 is
    // checked at launch) -- the 64-bit multiply this replaces cost three quarter-rate VALU instructions per load
    const unsigned short* kv_src[NLD2];
    unsigned kv_stride[NLD2];
    int kv_row[NLD2];
#pragma unroll
    for (int i = 0; i < NLD2; ++i) {
        const int item = tid + 256 * i;
        const bool is_v = item >= NCHUNK;
        const int ci = is_v ? item - NCHUNK : item;
        kv_row[i] = ci / CPR;
        kv_src[i] = (is_v ? vbase : kbase) + (ci % CPR) * 8;
        kv_stride[i] = (unsigned)(is_v ? P.v_stride : P.k_stride);
        // PAD: a chunk past the head (c >= dh / 8) re-reads the head's last chunk -- in bounds, no branch around the
        // prefetch -- and write_lds stores zeros in its place
        if constexpr (PAD) {
            if (ci % CPR >= dh / 8) kv_src[i] = (is_v ? vbase : kbase) + (dh / 8 - 1) * 8;
        }
    }
    auto load_regs = [&](int t) {
#pragma unroll
        for (int i = 0; i < NLD2; ++i) {
            int key = t * BKV + kv_row[i];
            key = key < len_k ? key : len_k - 1;                     // K: finite data for masked keys; V: in bounds only (write_lds zeroes it)
            const unsigned off = __umul24((unsigned)key, kv_stride[i]);
            kvreg[i] = *reinterpret_cast<const u32x4_t*>(kv_src[i] + off);
        }
    };
    auto write_lds = [&](int stage, int t) {
        char* sK = smem + stage * STAGE;
#pragma unroll
        for (int i = 0; i < NLD2; ++i) {
            const int item = tid + 256 * i;
            const bool is_v = item >= NCHUNK;
            const int ci = is_v ? item - NCHUNK : item;
            const int row = ci / CPR, c = ci % CPR;
            const int off = is_v ? K_TILE_BYTES + row * VROW + (c << 4)
                                 : row * K_ROW_BYTES + ((c ^ KLayout<DH>::swz(row)) << 4);
            // V rows past the sequence end are staged as zeros: their p is 0, and 0 x Inf = NaN would turn an Inf in the
            // replicated last V row into NaN (for finite V the same bits: the products are zeros either way)
            const bool zero = (PAD && c >= dh / 8) || (is_v && t * BKV + row >= len_k);
            *reinterpret_cast<u32x4_t*>(sK + off) = zero ? (u32x4_t){0u, 0u, 0u, 0u} : kvreg[i];
        }
        if (HwMask<DH>::value && tid < BKV)          // pad slot d = DH of every key row: 0 or the mask value
            *reinterpret_cast<u32x4_t*>(sK + tid * K_ROW_BYTES + ((CPR ^ ((tid >> 1) & 7)) << 4)) =
                mask_chunk<DT>(t * BKV + tid < len_k);
    };

    const int nkv = (len_k + BKV - 1) / BKV;
    load_regs(0);
    write_lds(0, 0);
    __syncthreads();

    // The last tile is peeled so that the loop body has no conditional loads / stores: with them hipcc's wait
    // bookkeeping turns conservative and drains the just-issued prefetch (s_waitcnt vmcnt(0)) before the first MFMA
    // of every tile.
    // a wave whose 16 * QG query rows all lie past the sequence (the last query block of a seq2reg window: 98 tokens =
    // one full block + 34 rows, i.e. one idle and one almost idle wave) still stages K/V and meets the barriers, but
    // computes nothing
    // (QG = 1 kernels only: in the 2-group ALiBi instantiation the extra branch costs 4 VGPRs, which is the third wave
    // per SIMD: 172 > 170)
    const bool active = QG > 1 || qb0 + wave * QG * 16 < len_q;       // wave-uniform
    for (int t = 0; t + 1 < nkv; ++t) {
        load_regs(t + 1);
        const char* sK = smem + (t & 1) * STAGE;
        if (active)
            attn_tile<DH, QG, ALIBI, DT, 4, (QL ? 2 : 0)>(sK, sK + K_TILE_BYTES, t * BKV, len_k, r, g, c, slope2, qf, q_pos, o,
                                                          m_run, l_acc);
        write_lds((t + 1) & 1, t + 1);
        __syncthreads();
    }
    if (active) {
        const int t = nkv - 1;
        const char* sK = smem + (t & 1) * STAGE;
        // short sequences (one query group per wave: seq2reg windows of 70-200 tokens, 2-4 tiles): the last tile in its
        // 16 / 32-key form when the remainder allows (a 100-token window: 64 + 36 keys; a 200-token chunk: 3 x 64 + 8)
        if (QG == 1 && len_k - t * BKV <= 32)
            attn_tile_short<DH, QG, ALIBI, DT, (QL ? 2 : 0)>(len_k - t * BKV, sK, sK + K_TILE_BYTES, t * BKV, len_k, r, g, c, slope2, qf,
                                               q_pos, o, m_run, l_acc);
        else
            attn_tile<DH, QG, ALIBI, DT, 4, (QL ? 2 : 0)>(sK, sK + K_TILE_BYTES, t * BKV, len_k, r, g, c, slope2, qf, q_pos, o,
                                                          m_run, l_acc);
    }

    // ---- normalise and store: lane (r,g) holds O[q = r][d = 16dt + 4g .. +3]
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        const float l = l_acc[qg][0];
        const float inv = 1.0f / l;
        if (q_abs[qg] < len_q) {
            unsigned short* op = P.out + (int64_t)(q_tok0 + q_abs[qg]) * P.o_stride + h * dh + 4 * g;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                u32x2_t pk;
                pk[0] = Op16<DT>::pack2(o[qg][dt][0] * inv, o[qg][dt][1] * inv);
                pk[1] = Op16<DT>::pack2(o[qg][dt][2] * inv, o[qg][dt][3] * inv);
                if (!PAD || 16 * dt + 4 * g < dh) *reinterpret_cast<u32x2_t*>(op + 16 * dt) = pk;   // 4 columns: all < dh or none
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Long query streams without positional bias at dh = 48 (the gene -> CRE cross attention: the T x G ~ 10^4 query rows of a
// gene against its ~10^3 CRE keys) on v_mfma_f32_32x32x16.  Why a second formulation: with 16x16x32 tiles this shape is
// bound by instruction ISSUE, not by the matrix pipe (per 64-key tile and wave 64 MFMAs x 8 issue cycles + 64 v_exp x 8 +
// ~300 other VALU x 4 = 2000 cycles against 1024 cycles of matrix work), and dh = 48 wastes a quarter of the QK^T MFMAs on
// padding the contraction to 64.  Here
//   S^T[key 32][query 32] = K . Q^T   A = 32 key rows x 16 d (ds_read_b128, three 16-deep steps = 48 exactly),
//                                     B = Q^T from registers; lane (q = lane & 31, h = lane >> 5) ends up with 16 keys of
//                                     ITS query per 32-key block: the row maximum is in-lane plus ONE half swap;
//   O^T[d 32][query 32] += V^T . P^T  A = V^T gathered by ds_read_b64_tr_b16 from the row-major V tile, B = P^T straight
//                                     from the score registers (regs 8s .. 8s+7 of a 32-key block are the 16-deep step s;
//                                     the k order inside a step is permuted identically on both operands);
//   the head dimension is padded to 64 on the OUTPUT side only, and the first padding column of V holds 1.0: row 48 of
//   O^T is then sum_k P = the softmax denominator -- the padding MFMAs do the row sums (no ones-fragment MFMAs).
// Per tile and wave (64 queries x 64 keys): 28 MFMAs of 32 cycles (12 QK^T + 16 PV) instead of 64 of 16, one permlane
// step per 32 queries instead of two per 16.
// LDS: K rows 112 B (96 + 16: the ds_read_b128 lane groups {0-3, 12-15, 20-27} then hit 16 distinct 16-byte slots),
// V rows 192 B (the 4 rows x 64 B a 32-lane half reads transposed fall on four distinct quarters of the 256-B bank row).
// ---------------------------------------------------------------------------------------------------------------------
// FAST (Q pre-scaled, AttnParams::q_log2): the accumulator of K . Q^T already is the base-2 logit, and the softmax runs
// WITHOUT a running maximum: p = exp2(s), O^T and the denominator (row 48) accumulate unnormalised -- per score one v_exp and
// half a v_cvt_pk instead of max3 + fma + exp + cvt (the kernel is bound by instruction issue; -14 % time).  Softmax is
// invariant under the offset, and fp32 / bf16 / fp16-with-offset carry the dynamic range as long as every row's largest
// logit stays inside (-100, +100 - log2(keys)): trained attention logits live within a few tens.  A block in which some
// valid row's denominator is not a normal number of moderate size (overflow, or every key underflowed) is detected at the
// end (one block-wide vote) and recomputed with the running-maximum form -- correctness never depends on the range, only
// the speed of such a block does.  The recomputation uses INTEGER offsets (ceil of the maximum): powers of two commute with
// the roundings, so both forms round the same probabilities.
// PAD: a head dim of 8 ... 40 in the 48 class (AttnParamsPad::dh): columns [dh, 48) of Q, K and V are zeros
template <int DT, int QB, bool FAST = false, bool PAD = false>
__global__ __launch_bounds__(256) void attn_x32_kernel(AttnArgs<PAD> P) {
    using frag_t = typename Op16<DT>::frag;
    constexpr int DH = 48, KSTEPS = 3, KROW = 112, VROW = 192;
    const int dh = PAD ? pad_dh(P) : DH;
    constexpr int K_TILE = BKV * KROW, V_TILE = BKV * VROW, STAGE = K_TILE + V_TILE;
    constexpr int CPR = DH / 8, NCHUNK = BKV * CPR, NLD2 = 2 * NCHUNK / 256;
    constexpr int BQ = 4 * QB * 32;
    static_assert(2 * NCHUNK % 256 == 0, "staging items must divide over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];       // 2 * STAGE bytes

    int seq, hd, qblk;
    if (!block_coords(P, seq, hd, qblk)) return;
    const int q_tok0 = P.cu_q[seq], len_q = P.cu_q[seq + 1] - q_tok0;
    const int k_tok0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k_tok0;
    const int qb0 = qblk * BQ;
    if (qb0 >= len_q) return;                         // block-uniform
    if (len_k <= 0) {
        zero_rows<DH, PAD>(P, q_tok0 + qb0, (len_q - qb0) < BQ ? (len_q - qb0) : BQ, hd);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 31, h = lane >> 5;

    // padding columns 48 .. 63 of every V row, both stages, once: column 48 = 1.0 (the denominator column), the rest 0
    if (tid < 2 * BKV) {
        char* vp = smem + (tid >> 6) * STAGE + K_TILE + (tid & 63) * VROW + DH * 2;
        *reinterpret_cast<u32x4_t*>(vp) = (u32x4_t){Op16<DT>::ONE, 0u, 0u, 0u};
        *reinterpret_cast<u32x4_t*>(vp + 16) = (u32x4_t){0u, 0u, 0u, 0u};
    }

    // ---- Q fragments (B operand): lane (q, h) holds Q[q][16 ks + 8 h .. + 7]
    frag_t qf[QB][KSTEPS];
    int q_abs[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        q_abs[qb] = qb0 + (wave * QB + qb) * 32 + ql;
        const int row = q_abs[qb] < len_q ? q_abs[qb] : len_q - 1;
        const unsigned short* qp = P.q + (int64_t)(q_tok0 + row) * P.q_stride + hd * dh + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            u32x4_t raw = (u32x4_t){0u, 0u, 0u, 0u};
            if (!PAD || 16 * ks + 8 * h < dh) raw = *reinterpret_cast<const u32x4_t*>(qp + 16 * ks);
            qf[qb][ks] = __builtin_bit_cast(frag_t, raw);
        }
    }
    const float c = P.scale_log2;
    f32x16_t o[QB][2];
    float m_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m_run[qb] = -INFINITY;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[qb][dt][i] = 0.f;
    }

    // ---- K/V tile staging: global -> registers -> LDS, one list of 2 * NCHUNK 16-byte items, NLD2 per thread (see
    // attn_fwd_kernel: no divergent branch around the prefetch)
    u32x4_t kvreg[NLD2];
    const unsigned short* kbase = P.k + (int64_t)k_tok0 * P.k_stride + hd * dh;
    const unsigned short* vbase = P.v + (int64_t)k_tok0 * P.v_stride + hd * dh;
    const unsigned short* kv_src[NLD2];
    unsigned kv_stride[NLD2];
    int kv_row[NLD2], kv_off[NLD2];
    bool kv_pad[NLD2];                                // PAD: the item is a chunk past the head (loads in bounds, stores zeros)
#pragma unroll
    for (int i = 0; i < NLD2; ++i) {
        const int item = tid + 256 * i;
        const bool is_v = item >= NCHUNK;
        const int ci = is_v ? item - NCHUNK : item;
        kv_row[i] = ci / CPR;
        kv_pad[i] = PAD && ci % CPR >= dh / 8;
        kv_src[i] = (is_v ? vbase : kbase) + (kv_pad[i] ? dh / 8 - 1 : ci % CPR) * 8;
        kv_stride[i] = (unsigned)(is_v ? P.v_stride : P.k_stride);
        kv_off[i] = is_v ? K_TILE + kv_row[i] * VROW + (ci % CPR) * 16 : kv_row[i] * KROW + (ci % CPR) * 16;
    }
    auto load_regs = [&](int t) {
#pragma unroll
        for (int i = 0; i < NLD2; ++i) {
            int key = t * BKV + kv_row[i];
            key = key < len_k ? key : len_k - 1;                     // K: finite data for masked keys; V: in bounds only (write_lds zeroes it)
            kvreg[i] = *reinterpret_cast<const u32x4_t*>(kv_src[i] + __umul24((unsigned)key, kv_stride[i]));
        }
    };
    auto write_lds = [&](int stage, int t) {
#pragma unroll
        for (int i = 0; i < NLD2; ++i) {
            // V rows past the sequence end are staged as zeros (p = 0 there, and 0 x Inf = NaN; see attn_fwd_kernel)
            const bool zero = kv_pad[i] || (tid + 256 * i >= NCHUNK && t * BKV + kv_row[i] >= len_k);
            *reinterpret_cast<u32x4_t*>(smem + stage * STAGE + kv_off[i]) = zero ? (u32x4_t){0u, 0u, 0u, 0u} : kvreg[i];
        }
    };

    // fragment addresses inside a stage
    const int k_off = ql * KROW + h * 16;                                           // + kb * 32 * KROW + ks * 32
    const int v_off = K_TILE + (4 * h + ((lane & 15) >> 2)) * VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    //                                                                              // + (32 kb + 16 s [+ 8]) * VROW + dt * 64

    // TAIL: the key tile may reach past len_k (only the last tile of a sequence; a compile-time flag, so that the
    // steady-state loop body carries no masking code at all)
    auto tile = [&](const char* st, int kb0, auto tail_c, auto fast_c) {
        constexpr bool TAIL = decltype(tail_c)::value;
        constexpr bool NOMAX = decltype(fast_c)::value;
        // ---- S^T = K . Q^T
        frag_t kf[2][KSTEPS];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
                kf[kb][ks] = *reinterpret_cast<const frag_t*>(st + k_off + kb * 32 * KROW + ks * 32);
        f32x16_t s[QB][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) s[qb][kb][i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) s[qb][kb] = Op16<DT>::mfma32(kf[kb][ks], qf[qb][ks], s[qb][kb]);
            }
        // V^T fragments of the whole tile: [kb][s][dt]
        frag_t vf[2][2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char* vp = st + v_off + (32 * kb + 16 * sx) * VROW + dt * 64;
                    const s16x4_t lo = lds_tr_read(vp);
                    const s16x4_t hi = lds_tr_read(vp + 8 * VROW);
                    vf[kb][sx][dt] = __builtin_bit_cast(frag_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                }
        // ---- online softmax: lane (q, h) holds keys kb0 + 32 kb + (i & 3) + 8 (i >> 2) + 4 h of query q
        float m_new[QB];
        bool moved = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            if (TAIL) {
                const int klim = len_k - kb0 - 4 * h;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        s[qb][kb][i] = (32 * kb + (i & 3) + 8 * (i >> 2)) < klim ? s[qb][kb][i] : -INFINITY;
            }
            if (NOMAX) continue;
            float ma = max3f(s[qb][0][0], s[qb][0][1], s[qb][0][2]);
            float mb = max3f(s[qb][1][0], s[qb][1][1], s[qb][1][2]);
#pragma unroll
            for (int i = 3; i + 1 < 16; i += 2) {
                ma = max3f(ma, s[qb][0][i], s[qb][0][i + 1]);
                mb = max3f(mb, s[qb][1][i], s[qb][1][i + 1]);
            }
            float mx = max3f(ma, mb, max2f(s[qb][0][15], s[qb][1][15]));
            if (P.q_log2) mx = __builtin_ceilf(mx);      // integer offsets whenever q carries the scale: the recomputation pass
                                                         // of the FAST kernel rounds what FAST rounds
            const unsigned u = __float_as_uint(mx);
            auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            m_new[qb] = max3f(m_run[qb], __uint_as_float(sw[0]), __uint_as_float(sw[1]));   // finite: tile 0 holds a valid key
            moved = moved || (m_new[qb] > m_run[qb]);
        }
        if (!NOMAX && __any(moved)) {                    // wave-uniform; rare after the first tiles of a sequence
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                const float alpha = __builtin_amdgcn_exp2f((m_run[qb] - m_new[qb]) * c);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) o[qb][dt] *= alpha;     // row 48 (the denominator) included
            }
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            if (NOMAX) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[qb][kb][i] = __builtin_amdgcn_exp2f(s[qb][kb][i]);
            } else {
                m_run[qb] = m_new[qb];
                const float mc = -m_new[qb] * c;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[qb][kb][i] = __builtin_amdgcn_exp2f(fmaf(s[qb][kb][i], c, mc));
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    u32x4_t pk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk[j] = Op16<DT>::pack2(s[qb][kb][8 * sx + 2 * j], s[qb][kb][8 * sx + 2 * j + 1]);
                    const frag_t pf = __builtin_bit_cast(frag_t, pk);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) o[qb][dt] = Op16<DT>::mfma32(vf[kb][sx][dt], pf, o[qb][dt]);
                }
        }
    };

    const int nkv = (len_k + BKV - 1) / BKV;
    const bool active = qb0 + wave * QB * 32 < len_q;                 // wave-uniform
    auto pass = [&](auto fast_c) {
        load_regs(0);
        write_lds(0, 0);
        __syncthreads();
        for (int t = 0; t + 1 < nkv; ++t) {
            load_regs(t + 1);
            if (active) tile(smem + (t & 1) * STAGE, t * BKV, std::false_type{}, fast_c);
            write_lds((t + 1) & 1, t + 1);
            __syncthreads();
        }
        if (active) tile(smem + ((nkv - 1) & 1) * STAGE, (nkv - 1) * BKV, std::true_type{}, fast_c);
    };
    if (FAST) {
        pass(std::true_type{});
        // the denominators (row d = 48: element 8 of the dt = 1 tile in the h = 0 lanes) of the block's valid rows
        bool bad = false;
        if (active && h == 0) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                // 2^-100 .. 2^100 (false for NaN).  fp16 P: overflow shows as inf; at the low end the largest p of a row must
                // still be a NORMAL half with room below it (subnormal P would pass a 2^-100 test with 4 significant bits).
                // The denominator bounds the largest p from below only through the key count, l <= len_k * p_max, so the
                // test is on the MEAN p: l > len_k * 2^-11 guarantees p_max > 2^-11 (8 times the smallest normal half)
                // however many keys share the sum -- thousands of keys at logits of -17 ... -20 add up to 2^-6 with every
                // P subnormal (round-3 advice).  Conservative for peaked rows (recomputed although fine): never wrong.
                const float l_min = DT == VF_F16 ? fmaxf(0.015625f, (float)len_k * 4.8828125e-4f) : 7.8886e-31f;
                const float l = o[qb][1][8];
                bad = bad || !(l > l_min && l < 1.2676e30f);
            }
        }
        if (__syncthreads_or(bad)) {                                  // block-uniform (also orders the LDS stages)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                m_run[qb] = -INFINITY;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) o[qb][dt][i] = 0.f;
            }
            pass(std::false_type{});
            __syncthreads();                                          // the stages become the output staging below
        }
    } else {
        pass(std::false_type{});
        __syncthreads();
    }

    // ---- normalise and store: lane (q, h) holds O[q][d = 32 dt + (i & 3) + 8 (i >> 2) + 4 h]; the denominator is row
    // d = 48 = element 8 of the dt = 1 tile in the h = 0 lane.
    // Wide form (16-byte aligned output rows): the wave's 32 QB x 48 block goes through LDS (the K / V stages
    // are free: every wave is behind the vote / the barrier that ends the pass) and leaves as whole 96-byte row segments, 16 bytes per lane,
    // ~11 rows per store instruction -- instead of 12 QB eight-byte stores per lane that each touch 32 rows (the store path of
    // the CU is shared with the K / V loads of the co-resident block).  Same values, same bits.
    const bool wide = ((reinterpret_cast<uintptr_t>(P.out) | (uintptr_t)(P.o_stride * 2)) & 15) == 0;
    constexpr int OPITCH = DH * 2 + 16;
    char* const oreg = smem + wave * (QB * 32 * OPITCH);
    static_assert(4 * QB * 32 * OPITCH <= 2 * STAGE, "the output staging must fit the K / V stages");
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const unsigned lu = __float_as_uint(o[qb][1][8]);
        auto sw = __builtin_amdgcn_permlane32_swap(lu, lu, false, false);
        const float inv = 1.0f / __uint_as_float(sw[0]);              // the lower half's value in both halves
        if (wide || q_abs[qb] < len_q) {
            unsigned short* op = wide ? reinterpret_cast<unsigned short*>(oreg + (qb * 32 + ql) * OPITCH) + 4 * h
                                      : P.out + (int64_t)(q_tok0 + q_abs[qb]) * P.o_stride + hd * dh + 4 * h;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int gq = 0; gq < (dt == 0 ? 4 : 2); ++gq) {
                    u32x2_t pk;
                    pk[0] = Op16<DT>::pack2(o[qb][dt][4 * gq] * inv, o[qb][dt][4 * gq + 1] * inv);
                    pk[1] = Op16<DT>::pack2(o[qb][dt][4 * gq + 2] * inv, o[qb][dt][4 * gq + 3] * inv);
                    if (!PAD || wide || 32 * dt + 8 * gq + 4 * h < dh) *reinterpret_cast<u32x2_t*>(op + 32 * dt + 8 * gq) = pk;
                }
        }
    }
    if (wide && active) {                                              // wave-local: a wave reads back only what it wrote
        constexpr int NCH = QB * 32 * (DH / 8), NIT = (NCH + 63) / 64;
        const int q_w0 = qb0 + wave * QB * 32;
        u32x4_t v[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int item = lane + 64 * i, row = item / (DH / 8), cc = item - row * (DH / 8);
            v[i] = *reinterpret_cast<const u32x4_t*>(oreg + (item < NCH ? row * OPITCH + cc * 16 : 0));
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int item = lane + 64 * i, row = item / (DH / 8), cc = item - row * (DH / 8);
            if (item < NCH && q_w0 + row < len_q && (!PAD || cc < dh / 8))
                *reinterpret_cast<u32x4_t*>(P.out + (int64_t)(q_tok0 + q_w0 + row) * P.o_stride + hd * dh + cc * 8) = v[i];
        }
    }
}

// Short sequences (<= 256 queries and keys: seq2reg windows, the gene stream): one block per (sequence, head).
// The whole K/V of the sequence is staged into LDS once (all loads issued before the first store: one load latency,
// no per-tile barriers) and is fetched once per (sequence, head) instead of once per 64-query block.
// Wave w owns the query groups w, w+4, ... (16 queries each), QG = ceil(max_seqlen_q / 64) of them, processed
// together so that every K / V fragment read from LDS feeds QG MFMAs.
// QL: q carries the softmax scale (AttnParams::q_log2) -> attn_tile mode 2 (integer running maxima), the arithmetic of the
// tiled kernels, which serve the same queries in other batch geometries.  (The no-maximum form of attn_x32_kernel was
// measured here too: -2 % on the gene stream's self attention -- this kernel waits for its loads, not for its exponentials --
// and it cannot be bit-identical to mode 2, whose s - m rounds; not kept.)
// PAD: a head dim below the class DH (AttnParamsPad::dh): chunks [dh / 8, CPR) are staged as zeros
template <int DH, int QG, bool ALIBI, int DT = VF_BF16, bool QL = false, bool PAD = false>
__global__ __launch_bounds__(256, (QG >= 2 ? 2 : 4)) void attn_short_kernel(AttnArgs<PAD> P, int k_rows) {
    constexpr int SM = QL ? 2 : 0;
    using frag_t = typename Op16<DT>::frag;
    const int dh = PAD ? pad_dh(P) : DH;
    constexpr int CPR = DH / 8;
    constexpr int NDT = DH / 16;
    constexpr int VROW = VLayout<DH>::ROW;
    constexpr int K_ROW_BYTES = KLayout<DH>::ROW, KS = KLayout<DH>::KS;
    static_assert(K_ROW_BYTES == 128, "the short-sequence kernel is written for dh <= 64");
    constexpr int MAXIT = 8;                                      // 256 rows x 8 chunk slots / 256 threads
    extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
    char* const sK0 = smem_dyn;
    char* const sV0 = smem_dyn + k_rows * K_ROW_BYTES;

    int seq, h, qblk;
    if (!block_coords(P, seq, h, qblk)) return;
    const int q_tok0 = P.cu_q[seq], len_q = P.cu_q[seq + 1] - q_tok0;
    const int k_tok0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k_tok0;
    if (len_q <= 0) return;
    if (len_k <= 0) {
        zero_rows<DH, PAD>(P, q_tok0, len_q, h);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nkv = (len_k + BKV - 1) / BKV;
    const int nchunks = nkv * BKV * 8;

    // ---- Q fragments of this wave's query groups (issued before the K/V loads so that both are in flight together)
    frag_t qf[QG][KS];
    int q_abs[QG];
    float q_pos[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        q_abs[qg] = (wave + 4 * qg) * 16 + r;
        const int row = q_abs[qg] < len_q ? q_abs[qg] : len_q - 1;
        const unsigned short* qp = P.q + (int64_t)(q_tok0 + row) * P.q_stride + h * dh;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int d0 = 32 * ks + 8 * g;
            u32x4_t raw = q_pad_chunk<DT>(d0, DH);
            if (d0 < dh) raw = *reinterpret_cast<const u32x4_t*>(qp + d0);
            qf[qg][ks] = *reinterpret_cast<frag_t*>(&raw);
        }
        q_pos[qg] = (float)(q_abs[qg] + (P.q_at_start ? 0 : len_k - len_q));
    }
    // ---- stage K (swizzled, zero pad chunks) and V; K rows >= len_k replicate the last key (masked later), V rows are zeros
    const unsigned short* kbase = P.k + (int64_t)k_tok0 * P.k_stride + h * dh;
    const unsigned short* vbase = P.v + (int64_t)k_tok0 * P.v_stride + h * dh;
    {
        u32x4_t kbuf[MAXIT], vbuf[MAXIT];
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int ci = tid + 256 * it;
            const int row = ci >> 3, cc = ci & 7;
            kbuf[it] = (HwMask<DH>::value && cc == CPR) ? mask_chunk<DT>(row < len_k) : (u32x4_t){0u, 0u, 0u, 0u};
            vbuf[it] = (u32x4_t){0u, 0u, 0u, 0u};
            if (ci < nchunks && cc < dh / 8) {
                const int key = row < len_k ? row : len_k - 1;
                kbuf[it] = *reinterpret_cast<const u32x4_t*>(kbase + (int64_t)key * P.k_stride + cc * 8);
                // (V rows past the sequence end stay zeros: p = 0 there, and 0 x Inf = NaN; see attn_fwd_kernel)
                if (row < len_k) vbuf[it] = *reinterpret_cast<const u32x4_t*>(vbase + (int64_t)key * P.v_stride + cc * 8);
            }
        }
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int ci = tid + 256 * it;
            const int row = ci >> 3, cc = ci & 7;
            if (ci < nchunks) {
                *reinterpret_cast<u32x4_t*>(sK0 + row * K_ROW_BYTES + ((cc ^ ((row >> 1) & 7)) << 4)) = kbuf[it];
                if (cc < CPR) *reinterpret_cast<u32x4_t*>(sV0 + row * VROW + (cc << 4)) = vbuf[it];
            }
        }
    }

    const float c = P.scale_log2;
    const float slope2 = ALIBI ? P.slopes[h] * 1.4426950408889634f : 0.f;
    f32x4_t o[QG][NDT];
    float m_run[QG];
    f32x4_t l_acc[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        m_run[qg] = -INFINITY;
        l_acc[qg] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[qg][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (wave * 16 >= len_q) return;                                // this wave owns no valid query (wave-uniform)

    // A wave whose LAST query group lies past the sequence (201 queries = 13 groups of 16 over 4 waves: waves 1-3 own 3
    // valid groups, wave 0 four) runs the tile function for one group fewer instead of computing a group of clamped
    // rows nobody stores: 19 % of the block's matrix and vector work at the gene stream's 201-token sequences.  The
    // arrays of the first QG - 1 groups are prefixes of the QG-group arrays.
    const bool last_group_valid = (wave + 4 * (QG - 1)) * 16 < len_q;             // wave-uniform
    // the last tile in its 16 / 32-key form when the remainder allows (201 keys = 3 tiles + 9 keys: 3/16 of the arithmetic)
    const int tl = nkv - 1, rem = len_k - tl * BKV;
    const int n_full = rem <= 32 ? tl : nkv;
    if (QG == 1 || last_group_valid) {
        for (int t = 0; t < n_full; ++t)
            attn_tile<DH, QG, ALIBI, DT, 4, SM>(sK0 + t * BKV * K_ROW_BYTES, sV0 + t * BKV * VROW, t * BKV, len_k, r, g, c,
                                                   slope2, qf, q_pos, o, m_run, l_acc);
        if (rem <= 32)
            attn_tile_short<DH, QG, ALIBI, DT, SM>(rem, sK0 + tl * BKV * K_ROW_BYTES, sV0 + tl * BKV * VROW, tl * BKV, len_k,
                                                   r, g, c, slope2, qf, q_pos, o, m_run, l_acc);
    } else {
        constexpr int Q1 = QG > 1 ? QG - 1 : 1;
        auto& qf1 = reinterpret_cast<const frag_t(&)[Q1][KS]>(qf);
        auto& q_pos1 = reinterpret_cast<const float(&)[Q1]>(q_pos);
        auto& o1 = reinterpret_cast<f32x4_t(&)[Q1][NDT]>(o);
        auto& m_run1 = reinterpret_cast<float(&)[Q1]>(m_run);
        auto& l_acc1 = reinterpret_cast<f32x4_t(&)[Q1]>(l_acc);
        for (int t = 0; t < n_full; ++t)
            attn_tile<DH, Q1, ALIBI, DT, 4, SM>(sK0 + t * BKV * K_ROW_BYTES, sV0 + t * BKV * VROW, t * BKV, len_k, r, g, c,
                                                   slope2, qf1, q_pos1, o1, m_run1, l_acc1);
        if (rem <= 32)
            attn_tile_short<DH, Q1, ALIBI, DT, SM>(rem, sK0 + tl * BKV * K_ROW_BYTES, sV0 + tl * BKV * VROW, tl * BKV, len_k,
                                                   r, g, c, slope2, qf1, q_pos1, o1, m_run1, l_acc1);
    }

#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        const float l = l_acc[qg][0];
        const float inv = 1.0f / l;
        if (q_abs[qg] < len_q) {
            unsigned short* op = P.out + (int64_t)(q_tok0 + q_abs[qg]) * P.o_stride + h * dh + 4 * g;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                u32x2_t pk;
                pk[0] = Op16<DT>::pack2(o[qg][dt][0] * inv, o[qg][dt][1] * inv);
                pk[1] = Op16<DT>::pack2(o[qg][dt][2] * inv, o[qg][dt][3] * inv);
                if (!PAD || 16 * dt + 4 * g < dh) *reinterpret_cast<u32x2_t*>(op + 16 * dt) = pk;
            }
        }
    }
}

// The same kernel for THREE resident blocks per CU (the gene stream's 201-token sequences).  attn_short_kernel at 4 query
// groups per wave needs 232 VGPRs and 57 KB of LDS: two blocks per CU, whose two long phases -- ~5 us waiting for 58 KB of
// Q / K / V at the latency this kernel's own traffic produces, ~6 us of tile arithmetic on the wave that owns 4 of the 13 query
// groups (profiles/r03_o_attn_short_phase_probe.log) -- hide behind each other and nothing else.  Here a wave makes TWO PASSES
// over the keys with 2 query groups each (<= 170 VGPRs: three waves per SIMD; the K / V fragments are read twice from LDS,
// which has the bandwidth), and the LDS image holds only the rows the tiles read -- keys rounded up to the tail tile's 16 /
// 32 / 64 for K and to 32 / 64 for V (201 keys: 208 K rows + 224 V rows = 47 KB) -- so three blocks fit: a third block's loads
// and a second computing wave per SIMD.  Arithmetic per query: attn_tile's, identical to every other kernel.
// NPASS = 1: sequences of <= 128 queries (seq2reg windows at dh = 64: one block per (window, head) instead of two 64-query
// blocks of the tiled kernel that each fetch K / V and wait for it).
// NPASS = 2 at dh = 64 (round 4): 129-256-token chunks (seq2reg's gene chunks), 62 KB image = two blocks per CU.  The register
// budget stays that of three waves per SIMD: at (256, 2) the compiler hoists loads up to 256 VGPRs + 47 spilled and the launch
// takes 2369 us instead of 1329 us (168 VGPRs, 12 spilled) -- profiles/r04_k.
// ROWS: Q / K / V rows are fetched through AttnParams::q_rows / kv_rows (one index load per row in front of the data loads).
// PAD: a head dim below the class DH (AttnParamsPad::dh; no row-map form)
template <int DH, bool ALIBI, int DT = VF_BF16, bool QL = false, int NPASS = 2, bool ROWS = false, bool PAD = false>
__global__ __launch_bounds__(256, 3) void attn_short2_kernel(AttnArgs<PAD> P, int k_rows) {
    static_assert(!(ROWS && PAD), "padded head dims have no row-map form");
    constexpr int SM = QL ? 2 : 0;
    using frag_t = typename Op16<DT>::frag;
    const int dh = PAD ? pad_dh(P) : DH;
    constexpr int CPR = DH / 8, NDT = DH / 16, QG = 2;
    constexpr int VROW = VLayout<DH>::ROW;
    constexpr int K_ROW_BYTES = KLayout<DH>::ROW, KS = KLayout<DH>::KS;
    static_assert(K_ROW_BYTES == 128, "the short-sequence kernel is written for dh <= 64");
    constexpr int MAXIT = 8;                                      // 256 rows x 8 chunk slots / 256 threads
    extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
    char* const sK0 = smem_dyn;
    char* const sV0 = smem_dyn + k_rows * K_ROW_BYTES;

    int seq, h, qblk;
    if (!block_coords(P, seq, h, qblk)) return;
    const int q_tok0 = P.cu_q[seq], len_q = P.cu_q[seq + 1] - q_tok0;
    const int k_tok0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k_tok0;
    if (len_q <= 0) return;
    if (len_k <= 0) {
        zero_rows<DH, PAD>(P, q_tok0, len_q, h);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nkv = (len_k + BKV - 1) / BKV;
    const int tl = nkv - 1, rem = len_k - tl * BKV;               // the last tile and the keys it holds
    const int n_full = rem <= 32 ? tl : nkv;
    const int rows_k = tl * BKV + (rem <= 16 ? 16 : rem <= 32 ? 32 : BKV);     // K rows the tiles read
    const int rows_v = tl * BKV + (rem <= 32 ? 32 : BKV);                      // V rows (a PV block spans 32 keys)

    // ---- Q fragments of all four query groups of this wave (issued before the K/V loads: everything in flight together)
    frag_t qf[NPASS][QG][KS];
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            const int qa = (wave + 4 * (QG * ps + qg)) * 16 + r;
            const int row = qa < len_q ? qa : len_q - 1;
            const int64_t qrow = (ROWS && P.q_rows) ? P.q_rows[q_tok0 + row] : (int64_t)(q_tok0 + row);
            const unsigned short* qp = P.q + qrow * P.q_stride + h * dh;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int d0 = 32 * ks + 8 * g;
                u32x4_t raw = q_pad_chunk<DT>(d0, DH);
                if (d0 < dh) raw = *reinterpret_cast<const u32x4_t*>(qp + d0);
                qf[ps][qg][ks] = *reinterpret_cast<frag_t*>(&raw);
            }
        }
    // ---- stage K (swizzled, zero pad chunks) and V; K rows >= len_k replicate the last key (masked later), V rows are zeros
    const unsigned short* kbase = P.k + h * dh;
    const unsigned short* vbase = P.v + h * dh;
    {
        u32x4_t kbuf[MAXIT], vbuf[MAXIT];
        int64_t src[MAXIT];                          // source row of every staged row: all index loads in flight before the data loads
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int row = (tid + 256 * it) >> 3;
            const int key = row < len_k ? row : len_k - 1;
            src[it] = (ROWS && P.kv_rows) ? (row < rows_v ? P.kv_rows[k_tok0 + key] : 0) : (int64_t)(k_tok0 + key);
        }
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int ci = tid + 256 * it;
            const int row = ci >> 3, cc = ci & 7;
            kbuf[it] = (HwMask<DH>::value && cc == CPR) ? mask_chunk<DT>(row < len_k) : (u32x4_t){0u, 0u, 0u, 0u};
            vbuf[it] = (u32x4_t){0u, 0u, 0u, 0u};
            if (row < rows_v && cc < dh / 8) {
                if (row < rows_k) kbuf[it] = *reinterpret_cast<const u32x4_t*>(kbase + src[it] * P.k_stride + cc * 8);
                // (V rows past the sequence end stay zeros: p = 0 there, and 0 x Inf = NaN; see attn_fwd_kernel)
                if (row < len_k) vbuf[it] = *reinterpret_cast<const u32x4_t*>(vbase + src[it] * P.v_stride + cc * 8);
            }
        }
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int ci = tid + 256 * it;
            const int row = ci >> 3, cc = ci & 7;
            if (row < rows_k) *reinterpret_cast<u32x4_t*>(sK0 + row * K_ROW_BYTES + ((cc ^ ((row >> 1) & 7)) << 4)) = kbuf[it];
            if (row < rows_v && cc < CPR) *reinterpret_cast<u32x4_t*>(sV0 + row * VROW + (cc << 4)) = vbuf[it];
        }
    }
    const float c = P.scale_log2;
    const float slope2 = ALIBI ? P.slopes[h] * 1.4426950408889634f : 0.f;
    __syncthreads();

#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int g0 = wave + 4 * QG * ps;                         // this pass's first query group (wave-uniform)
        if (g0 * 16 >= len_q) break;
        int q_abs[QG];
        float q_pos[QG], m_run[QG];
        f32x4_t o[QG][NDT], l_acc[QG];
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            q_abs[qg] = (g0 + 4 * qg) * 16 + r;
            q_pos[qg] = (float)(q_abs[qg] + (P.q_at_start ? 0 : len_k - len_q));
            m_run[qg] = -INFINITY;
            l_acc[qg] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[qg][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        }
        if ((g0 + 4) * 16 < len_q) {                               // both groups hold valid queries
            for (int t = 0; t < n_full; ++t)
                attn_tile<DH, QG, ALIBI, DT, 4, SM>(sK0 + t * BKV * K_ROW_BYTES, sV0 + t * BKV * VROW, t * BKV, len_k, r, g, c,
                                                       slope2, qf[ps], q_pos, o, m_run, l_acc);
            if (rem <= 32)
                attn_tile_short<DH, QG, ALIBI, DT, SM>(rem, sK0 + tl * BKV * K_ROW_BYTES, sV0 + tl * BKV * VROW, tl * BKV, len_k,
                                                       r, g, c, slope2, qf[ps], q_pos, o, m_run, l_acc);
        } else {
            auto& qf1 = reinterpret_cast<const frag_t(&)[1][KS]>(qf[ps]);
            auto& q_pos1 = reinterpret_cast<const float(&)[1]>(q_pos);
            auto& o1 = reinterpret_cast<f32x4_t(&)[1][NDT]>(o);
            auto& m_run1 = reinterpret_cast<float(&)[1]>(m_run);
            auto& l_acc1 = reinterpret_cast<f32x4_t(&)[1]>(l_acc);
            for (int t = 0; t < n_full; ++t)
                attn_tile<DH, 1, ALIBI, DT, 4, SM>(sK0 + t * BKV * K_ROW_BYTES, sV0 + t * BKV * VROW, t * BKV, len_k, r, g, c,
                                                      slope2, qf1, q_pos1, o1, m_run1, l_acc1);
            if (rem <= 32)
                attn_tile_short<DH, 1, ALIBI, DT, SM>(rem, sK0 + tl * BKV * K_ROW_BYTES, sV0 + tl * BKV * VROW, tl * BKV, len_k,
                                                      r, g, c, slope2, qf1, q_pos1, o1, m_run1, l_acc1);
        }
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            const float inv = 1.0f / l_acc[qg][0];
            if (q_abs[qg] < len_q) {
                unsigned short* op = P.out + (int64_t)(q_tok0 + q_abs[qg]) * P.o_stride + h * dh + 4 * g;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    u32x2_t pk;
                    pk[0] = Op16<DT>::pack2(o[qg][dt][0] * inv, o[qg][dt][1] * inv);
                    pk[1] = Op16<DT>::pack2(o[qg][dt][2] * inv, o[qg][dt][3] * inv);
                    if (!PAD || 16 * dt + 4 * g < dh) *reinterpret_cast<u32x2_t*>(op + 16 * dt) = pk;
                }
            }
        }
    }
}

// Only attn_short2_kernel's ROWS instantiations read AttnParams::q_rows / kv_rows: every other launcher refuses a row map
// instead of silently attending over the wrong rows (round-5 advice).
static int no_row_map(const AttnParams& P, const char* kernel) {
    if (!P.q_rows && !P.kv_rows) return VF_OK;
    vf_set_error("vf_attn_varlen_fwd_rows: %s has no row-map form (ask vf_attn_rows_supported first)", kernel);
    return VF_ERR_INVALID_ARG;
}

// fills the grid decomposition of block_coords; returns the (padded) 1-D grid size
static unsigned set_grid(AttnParams& P, int n_seq, int nqb) {
    const long total = (long)n_seq * P.H * nqb;
    P.nqb = nqb;
    P.total = (int)total;
    P.chunk = (int)((total + 7) / 8);
    return 8u * (unsigned)P.chunk;
}

// dynamic LDS of the tiled kernel: two (K tile + V tile) stages
template <int DH> constexpr int attn_fwd_lds() { return 2 * (KLayout<DH>::TILE + VLayout<DH>::TILE); }

template <int DH, int QG, bool ALIBI, int DT, bool QL, bool PAD>
int launch_fwd_k(const AttnParamsPad& P, dim3 grid, hipStream_t st) {
    auto kern = attn_fwd_kernel<DH, QG, ALIBI, DT, QL, PAD>;
    constexpr int lds = attn_fwd_lds<DH>();
    if (lds > 65536) {                             // dh >= 128: above the default dynamic-LDS limit (dh 256: 132 KiB)
        static bool attr_set[VF_MAX_DEVICES] = {};
        const int dev = vf_current_device();
        if (dev < 0 || !attr_set[dev]) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
                hipSuccess) {
                (void)hipGetLastError();
                vf_set_error("vf_attn_varlen_fwd: cannot reserve %d bytes of LDS", lds);
                return VF_ERR_LAUNCH;
            }
            if (dev >= 0) attr_set[dev] = true;
        }
    }
    vf_note_kernel(1, QG == 1 ? "attn_fwd_kernel<64-query blocks>" : QG == 2 ? "attn_fwd_kernel<128-query blocks>" : "attn_fwd_kernel<256-query blocks>");
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, static_cast<const AttnArgs<PAD>&>(P));
    VF_CHECK_LAUNCH("vf_attn_varlen_fwd");
    return VF_OK;
}

// q carrying the softmax scale (AttnParams::q_log2) selects the integer-maximum instantiation (attn_tile mode 2)
template <int DH, int QG, bool ALIBI, int DT, bool PAD = false>
int launch_fwd(const AttnParamsPad& P, dim3 grid, hipStream_t st) {
    if (const int rc = no_row_map(P, "attn_fwd_kernel")) return rc;
    if (P.q_log2) return launch_fwd_k<DH, QG, ALIBI, DT, true, PAD>(P, grid, st);
    return launch_fwd_k<DH, QG, ALIBI, DT, false, PAD>(P, grid, st);
}

template <int DH, int QG, bool ALIBI, int DT, bool QL, bool PAD>
int launch_short_k(AttnParamsPad P, int n_seq, int max_k, hipStream_t st) {
    const int k_rows = ((max_k + BKV - 1) / BKV) * BKV;
    const int lds = k_rows * (KLayout<DH>::ROW + VLayout<DH>::ROW);
    auto kern = attn_short_kernel<DH, QG, ALIBI, DT, QL, PAD>;
    static bool attr_set[VF_MAX_DEVICES] = {};    // the attribute is per device (and per instantiation)
    const int dev = vf_current_device();
    if (dev < 0 || !attr_set[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                256 * (KLayout<DH>::ROW + VLayout<DH>::ROW)) != hipSuccess) {
            (void)hipGetLastError();
            vf_set_error("vf_attn_varlen_fwd: cannot reserve LDS");
            return VF_ERR_LAUNCH;
        }
        if (dev >= 0) attr_set[dev] = true;
    }
    const unsigned nblk = set_grid(P, n_seq, 1);
    vf_note_kernel(1, "attn_short_kernel");
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), lds, st, static_cast<const AttnArgs<PAD>&>(P), k_rows);
    VF_CHECK_LAUNCH("vf_attn_varlen_fwd");
    return VF_OK;
}

// rows of the LDS image for sequences of at most max_k keys (monotone in max_k: a shorter sequence never reads beyond them)
static inline void short2_rows(int max_k, int& kr, int& vr) {
    const int tl = (max_k - 1) / BKV, rem = max_k - tl * BKV;
    kr = tl * BKV + (rem <= 16 ? 16 : rem <= 32 ? 32 : BKV);
    vr = tl * BKV + (rem <= 32 ? 32 : BKV);
}

template <int DH, bool ALIBI, int DT, bool QL, int NPASS, bool ROWS = false, bool PAD = false>
int launch_short2_k(AttnParamsPad P, int n_seq, int max_k, hipStream_t st) {
    int kr, vr;
    short2_rows(max_k, kr, vr);
    const int lds = kr * KLayout<DH>::ROW + vr * VLayout<DH>::ROW;
    auto kern = attn_short2_kernel<DH, ALIBI, DT, QL, NPASS, ROWS, PAD>;
    static bool attr_set[VF_MAX_DEVICES] = {};
    const int dev = vf_current_device();
    if (dev < 0 || !attr_set[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                256 * (KLayout<DH>::ROW + VLayout<DH>::ROW)) != hipSuccess) {
            (void)hipGetLastError();
            vf_set_error("vf_attn_varlen_fwd: cannot reserve LDS");
            return VF_ERR_LAUNCH;
        }
        if (dev >= 0) attr_set[dev] = true;
    }
    const unsigned nblk = set_grid(P, n_seq, 1);
    vf_note_kernel(1, ROWS ? (NPASS == 1 ? "attn_short2_kernel<1 pass,rows>" : "attn_short2_kernel<2 passes,rows>")
                           : (NPASS == 1 ? "attn_short2_kernel<1 pass>" : "attn_short2_kernel<2 passes>"));
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), lds, st, static_cast<const AttnArgs<PAD>&>(P), kr);
    VF_CHECK_LAUNCH("vf_attn_varlen_fwd");
    return VF_OK;
}

template <int DH, bool ALIBI, int DT, int NPASS = 2, bool PAD = false>
int launch_short2(AttnParamsPad P, int n_seq, int max_k, hipStream_t st) {
    if (P.q_rows || P.kv_rows) {                 // only the model's call form (pre-scaled q) has a row-map instantiation
        if constexpr (!PAD && ((DH == 64 && !ALIBI) || (DH == 48 && ALIBI && NPASS == 2))) {
            if (P.q_log2) return launch_short2_k<DH, ALIBI, DT, true, NPASS, true>(P, n_seq, max_k, st);
        }
        vf_set_error("vf_attn_varlen_fwd_rows: no row-map kernel for this geometry (ask vf_attn_rows_supported first)");
        return VF_ERR_INVALID_ARG;
    }
    if (P.q_log2) return launch_short2_k<DH, ALIBI, DT, true, NPASS, false, PAD>(P, n_seq, max_k, st);
    return launch_short2_k<DH, ALIBI, DT, false, NPASS, false, PAD>(P, n_seq, max_k, st);
}

template <int DH, int QG, bool ALIBI, int DT, bool PAD = false>
int launch_short(AttnParamsPad P, int n_seq, int max_k, hipStream_t st) {
    if (const int rc = no_row_map(P, "attn_short_kernel")) return rc;
    if (P.q_log2) return launch_short_k<DH, QG, ALIBI, DT, true, PAD>(P, n_seq, max_k, st);
    return launch_short_k<DH, QG, ALIBI, DT, false, PAD>(P, n_seq, max_k, st);
}

template <int DT, int QB, bool PAD = false>
int launch_x32(const AttnParamsPad& P, dim3 grid, hipStream_t st) {
    if (const int rc = no_row_map(P, "attn_x32_kernel")) return rc;
    constexpr int lds = 2 * BKV * (112 + 192);
    vf_note_kernel(1, QB == 2 ? "attn_x32_kernel<64 queries per wave>" : "attn_x32_kernel<32 queries per wave>");
    const AttnArgs<PAD>& A = P;
    if (P.q_log2) hipLaunchKernelGGL((attn_x32_kernel<DT, QB, true, PAD>), grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL((attn_x32_kernel<DT, QB, false, PAD>), grid, dim3(256), lds, st, A);
    VF_CHECK_LAUNCH("vf_attn_varlen_fwd");
    return VF_OK;
}

// Geometries the row-map form (AttnParams::q_rows / kv_rows) serves: exactly those launch_attn sends to attn_short2_kernel
// in the model's call form -- seq2reg windows / chunks (dh 64, no bias) and the gene stream's self attention (dh 48, ALiBi,
// 129-256 tokens).  Everything else gathers the rows first (vf_gather_rows_bf16) and calls the plain entry: same bits.
static bool rows_supported(int dh, bool alibi, long n_seq, int H, int max_q, int max_k, bool q_log2) {
    if (!q_log2 || max_q <= 0 || max_k <= 0 || max_q > 256 || max_k > 256) return false;
    int kr, vr;
    short2_rows(max_k, kr, vr);
    // (exactly launch_attn's conditions, in its order: a geometry it sends elsewhere has no row map)
    if (dh == 48 && alibi)
        return max_q > 128 && 3 * (kr * KLayout<48>::ROW + vr * VLayout<48>::ROW) <= 160 * 1024;
    if (dh == 64 && !alibi) {
        if (n_seq * H < 1024) return false;
        const int image = kr * KLayout<64>::ROW + vr * VLayout<64>::ROW;
        if (max_q <= 128 && max_k <= 128) return 3 * image <= 160 * 1024;
        if (max_q > 128) return 2 * image <= 160 * 1024;          // (<= 256 both: checked above)
        return false;                                               // max_q <= 128 < max_k: the tiled kernel serves it
    }
    return false;
}

// PAD: DH is the class of the true head dim P.dh (vf_attn_varlen_fwd_v3).  The routing below is the class's, unchanged, so a
// padded head dim reaches the same kernel with the same block shape as a class-dh call of the same geometry.  The row-map
// check keys on the TRUE head dim (rows_supported has no padded entries, as vf_attn_rows_supported reports).
template <int DH, bool ALIBI, int DT, bool PAD = false>
int launch_attn(AttnParamsPad P, int n_seq, int max_q, int max_k, hipStream_t st) {
    const int dh = PAD ? P.dh : DH;
    if ((P.q_rows || P.kv_rows) && !rows_supported(dh, ALIBI, n_seq, P.H, max_q, max_k, P.q_log2 != 0)) {
        vf_set_error("vf_attn_varlen_fwd_rows: no row-map kernel for dh=%d alibi=%d n_seq=%d H=%d max_q=%d max_k=%d "
                     "(vf_attn_rows_supported says which geometries have one; gather the rows first otherwise)",
                     dh, (int)ALIBI, n_seq, P.H, max_q, max_k);
        return VF_ERR_INVALID_ARG;
    }
    // Measured on MI355X (scripts/attn_bench.py, 8 genes): the one-block-per-(sequence, head) kernel wins for the gene
    // stream (201-token sequences, dh 48: 396 vs 485 us); for seq2reg windows / chunks (dh 64, <= 200 tokens) the tiled
    // kernel with 64-query blocks is faster (460 vs 613 us on 200-token chunks: more blocks in flight, fewer registers;
    // the K/V re-reads of its query blocks hit the XCD's L2 thanks to block_coords).
    // dh = 48 without positional bias (every cross attention of the modulator): ONE kernel for every geometry, so that a
    // gene's result cannot depend on the batch it is evaluated in (the query-block size only changes which wave owns a
    // query, never the arithmetic of a query: tests test_cfg3 / test_headline batch independence at 1e-5).  64 queries
    // per wave once that leaves >= 8 blocks per CU (the batched gene -> CRE cross attention), else 32 (3 waves / SIMD).
    if constexpr (DH == 48 && !ALIBI) {
        if ((long)n_seq * P.H * ((max_q + 255) / 256) >= 2048)
            return launch_x32<DT, 2, PAD>(P, dim3(set_grid(P, n_seq, (max_q + 255) / 256)), st);
        return launch_x32<DT, 1, PAD>(P, dim3(set_grid(P, n_seq, (max_q + 127) / 128)), st);
    }
    if constexpr (DH <= 48) {
        if (max_q > 128 && max_q <= 256 && max_k <= 256) {
            // three resident blocks per CU (two passes of 2 query groups, trimmed LDS image) once the image leaves room
            // for them
            int kr, vr;
            short2_rows(max_k, kr, vr);
            if (3 * (kr * KLayout<DH>::ROW + vr * VLayout<DH>::ROW) <= 160 * 1024)
                return launch_short2<DH, ALIBI, DT, 2, PAD>(P, n_seq, max_k, st);
            if (max_q <= 192) return launch_short<DH, 3, ALIBI, DT, PAD>(P, n_seq, max_k, st);
            return launch_short<DH, 4, ALIBI, DT, PAD>(P, n_seq, max_k, st);
        }
    }
    if constexpr (DH == 64 || DH == 32) {
        // seq2reg windows (<= 128 tokens at dh = 64: a 36 KB image): one block per (window, head) with the whole K / V in
        // LDS instead of two 64-query blocks that each fetch K / V and wait for it.
        // dh = 32 (a tokenizer geometry the real checkpoint might have, scripts/s2r_dims_sweep.py) takes the same kernel
        // since round 6: the tiled kernel ran its windows at 3.2 TB/s against 4.1 for dh = 64.
        if (max_q <= 128 && max_k <= 128 && (long)n_seq * P.H >= 1024) {
            int kr, vr;
            short2_rows(max_k, kr, vr);
            if (3 * (kr * KLayout<DH>::ROW + vr * VLayout<DH>::ROW) <= 160 * 1024)
                return launch_short2<DH, ALIBI, DT, 1, PAD>(P, n_seq, max_k, st);
        }
        // 129-256-token chunks (seq2reg's 200-token gene chunks): the same kernel in its two-pass form, one block per (chunk,
        // head) with a 62 KB image (two resident blocks per CU) instead of four 64-query blocks of the tiled kernel that each
        // stage all keys: 1544 -> 1329 us per launch at 32 genes, bit-identical (profiles/r04_k)
        if (DH == 64 && max_q > 128 && max_q <= 256 && max_k <= 256 && (long)n_seq * P.H >= 1024) {
            int kr, vr;
            short2_rows(max_k, kr, vr);
            if (2 * (kr * KLayout<DH>::ROW + vr * VLayout<DH>::ROW) <= 160 * 1024)
                return launch_short2<DH, ALIBI, DT, 2, PAD>(P, n_seq, max_k, st);
        }
    }
    // long query streams: 2 query groups per wave (halves K/V LDS traffic per MFMA; for seq2reg windows, 70-200 queries,
    // 128-query blocks measured the same as 64-query blocks: 800 / 428 us either way, the kernel runs at 4 TB/s there);
    // short ones (seq2reg windows, gene stream): 64-query blocks to limit tail waste.
    // 2 query groups per wave only when that still leaves >= 4 blocks per CU (measured: CRE stream, 256 blocks, is
    // 15% faster with 64-query blocks; the 10^4-query gene->CRE cross attention is 17% faster with 128-query blocks).
    // dh = 128 (not a shape of the shipped model) always takes one query group per wave; dh = 96: below.
    if constexpr (DH <= 64) {
        if (max_q > 256 && (long)n_seq * P.H * ((max_q + 127) / 128) >= 1024) {
            const dim3 grid(set_grid(P, n_seq, (max_q + 127) / 128));
            // 4 query groups per wave (256-query blocks) once that still leaves >= 8 blocks per CU: every K/V fragment
            // read feeds 4 MFMAs (gene->CRE cross attention at 8 genes: 948 vs 993 us; no gain at one gene, 1376 blocks).
            // (That geometry now returns through attn_x32_kernel above, so this branch is not taken; its kernels stay in the
            // library until a change of its own removes them.)
            if constexpr (DH == 48 && !ALIBI) {
                if ((long)n_seq * P.H * ((max_q + 255) / 256) >= 2048)
                    return launch_fwd<48, 4, false, DT, PAD>(P, dim3(set_grid(P, n_seq, (max_q + 255) / 256)), st);
            }
            return launch_fwd<DH, 2, ALIBI, DT, PAD>(P, grid, st);
        }
    }
    if constexpr (DH == 96) {
        // dh = 96 (a tokenizer geometry the real checkpoint might have, scripts/s2r_dims_sweep.py): windows of 65-128 tokens
        // as ONE 128-query block per (window, head) -- two 64-query blocks would each stage all keys: 3.0 -> 3.5 TB/s.  (At
        // dh = 128 the two-group form needs all 256 VGPRs, one wave per SIMD, and is slower: 3.4 -> 3.1 TB/s.)
        if (max_q > 64 && max_q <= 128 && (long)n_seq * P.H >= 1024)
            return launch_fwd<DH, 2, ALIBI, DT, PAD>(P, dim3(set_grid(P, n_seq, 1)), st);
    }
    // dh 192 / 256 (padded classes only): the tiled kernel, one query group per wave -- two stages of K / V are 100 / 132 KiB
    // of LDS (one block per CU), and the O accumulators alone are 48 / 64 registers per query group
    return launch_fwd<DH, 1, ALIBI, DT, PAD>(P, dim3(set_grid(P, n_seq, (max_q + 63) / 64)), st);
}

}  // namespace

static bool legacy_dh(int dh) { return dh == 32 || dh == 48 || dh == 64 || dh == 96 || dh == 128; }

// any_dh (vf_attn_varlen_fwd_v3): every multiple of 8 in [8, 256]; the five class head dims take the same path as without it
template <int DT>
static int attn_dispatch(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                         int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                         const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                         int dh, const float* alibi_slopes, float scale, int flags, void* stream,
                         const int64_t* q_rows = nullptr, const int64_t* kv_rows = nullptr, bool any_dh = false) {
    const int q_at_start = flags & VF_ATTN_Q_AT_START, q_log2 = (flags & VF_ATTN_Q_LOG2) ? 1 : 0;
    VF_REQUIRE((flags & ~(VF_ATTN_Q_AT_START | VF_ATTN_Q_LOG2)) == 0, "vf_attn_varlen_fwd: unknown flag bits 0x%x", flags);
    VF_REQUIRE(q && k && v && out && cu_seqlens_q, "vf_attn_varlen_fwd: null pointer");
    if (any_dh)
        VF_REQUIRE(dh >= 8 && dh <= 256 && dh % 8 == 0,
                   "vf_attn_varlen_fwd_v3: head_dim %d not supported (a multiple of 8 in [8, 256])", dh);
    else
        VF_REQUIRE(legacy_dh(dh), "vf_attn_varlen_fwd: head_dim %d not supported (32/48/64/96/128)", dh);
    VF_REQUIRE(H > 0 && H <= 65535 && n_seq >= 0, "vf_attn_varlen_fwd: H=%d n_seq=%d out of range", H, n_seq);
    VF_REQUIRE((long)n_seq * H * ((max_seqlen_q + 63) / 64) < (1L << 31) - 8,
               "vf_attn_varlen_fwd: n_seq * H * ceil(max_seqlen_q / 64) exceeds the grid limit");
    VF_REQUIRE(q_stride % 8 == 0 && k_stride % 8 == 0 && v_stride % 8 == 0 && o_stride % 4 == 0,
               "vf_attn_varlen_fwd: row strides must keep 16-byte alignment");
    VF_REQUIRE(((uintptr_t)q % 16 == 0) && ((uintptr_t)k % 16 == 0) && ((uintptr_t)v % 16 == 0) && ((uintptr_t)out % 8 == 0),
               "vf_attn_varlen_fwd: pointers must be 16-byte aligned");
    if (n_seq == 0 || max_seqlen_q <= 0 || max_seqlen_k <= 0) return VF_OK;
    VF_REQUIRE(max_seqlen_k < (1 << 24) && k_stride < (1 << 24) && v_stride < (1 << 24) &&
                   (int64_t)max_seqlen_k * (k_stride > v_stride ? k_stride : v_stride) < (1LL << 31),
               "vf_attn_varlen_fwd: max_seqlen_k=%d, k_stride=%ld, v_stride=%ld: each must stay below 2^24 and max_seqlen_k * "
               "row stride below 2^31 elements (the tiled kernels form the key offset with a 24-bit multiply)",
               max_seqlen_k, (long)k_stride, (long)v_stride);
    AttnParamsPad P;
    P.q = (const unsigned short*)q; P.k = (const unsigned short*)k; P.v = (const unsigned short*)v;
    P.out = (unsigned short*)out;
    P.q_stride = q_stride; P.k_stride = k_stride; P.v_stride = v_stride; P.o_stride = o_stride;
    P.cu_q = cu_seqlens_q; P.cu_k = cu_seqlens_k ? cu_seqlens_k : cu_seqlens_q;
    P.slopes = alibi_slopes; P.scale_log2 = q_log2 ? 1.0f : scale * 1.4426950408889634f; P.H = H;
    P.q_at_start = q_at_start ? 1 : 0; P.q_log2 = q_log2;
    P.q_rows = q_rows; P.kv_rows = kv_rows;
    P.dh = dh;
    hipStream_t st = (hipStream_t)stream;
    const bool alibi = alibi_slopes != nullptr;
    if (!legacy_dh(dh)) {                            // a padded class (any_dh only)
#define VF_PAD(C_) return alibi ? launch_attn<C_, true, DT, true>(P, n_seq, max_seqlen_q, max_seqlen_k, st) \
                                : launch_attn<C_, false, DT, true>(P, n_seq, max_seqlen_q, max_seqlen_k, st)
        if (dh <= 32) VF_PAD(32);
        if (dh <= 48) VF_PAD(48);
        if (dh <= 64) VF_PAD(64);
        if (dh <= 96) VF_PAD(96);
        if (dh <= 128) VF_PAD(128);
        if (dh <= 192) VF_PAD(192);
        VF_PAD(256);
#undef VF_PAD
    }
    switch (dh) {
        case 32: return alibi ? launch_attn<32, true, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st) : launch_attn<32, false, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st);
        case 48: return alibi ? launch_attn<48, true, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st) : launch_attn<48, false, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st);
        case 64: return alibi ? launch_attn<64, true, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st) : launch_attn<64, false, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st);
        case 96: return alibi ? launch_attn<96, true, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st) : launch_attn<96, false, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st);
        default: return alibi ? launch_attn<128, true, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st) : launch_attn<128, false, DT>(P, n_seq, max_seqlen_q, max_seqlen_k, st);
    }
}

extern "C" int vf_attn_varlen_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                  int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                                  const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                                  int dh, const float* alibi_slopes, float scale, void* stream) {
    return attn_dispatch<VF_BF16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                         max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, 0, stream);
}

extern "C" int vf_attn_varlen_fwd_qstart(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                         int64_t k_stride, int64_t v_stride, int64_t o_stride,
                                         const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int n_seq,
                                         int max_seqlen_q, int max_seqlen_k, int H, int dh, const float* alibi_slopes,
                                         float scale, void* stream) {
    return attn_dispatch<VF_BF16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                         max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, 1, stream);
}

extern "C" int vf_attn_varlen_fwd_f16(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                      int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                                      const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                                      int dh, const float* alibi_slopes, float scale, void* stream) {
    return attn_dispatch<VF_F16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                 max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, 0, stream);
}

extern "C" int vf_attn_varlen_fwd_qstart_f16(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                             int64_t k_stride, int64_t v_stride, int64_t o_stride,
                                             const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int n_seq,
                                             int max_seqlen_q, int max_seqlen_k, int H, int dh, const float* alibi_slopes,
                                             float scale, void* stream) {
    return attn_dispatch<VF_F16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                 max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, 1, stream);
}

extern "C" int vf_attn_varlen_fwd_v2(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                     int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                                     const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                                     int dh, const float* alibi_slopes, float scale, int operand_dtype, int flags,
                                     void* stream) {
    if (operand_dtype == VF_BF16)
        return attn_dispatch<VF_BF16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                      max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream);
    VF_REQUIRE(operand_dtype == VF_F16, "vf_attn_varlen_fwd_v2: operand_dtype must be VF_BF16 or VF_F16");
    return attn_dispatch<VF_F16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                 max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream);
}

extern "C" int vf_attn_varlen_fwd_v3(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                     int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                                     const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                                     int dh, const float* alibi_slopes, float scale, int operand_dtype, int flags,
                                     void* stream) {
    if (operand_dtype == VF_BF16)
        return attn_dispatch<VF_BF16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                      max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream, nullptr, nullptr, true);
    VF_REQUIRE(operand_dtype == VF_F16, "vf_attn_varlen_fwd_v3: operand_dtype must be VF_BF16 or VF_F16");
    return attn_dispatch<VF_F16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                 max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream, nullptr, nullptr, true);
}

// ---------------------------------------------------------------------------------------------------------------------
// Cross attention against keys that are COPIES OF A FEW DISTINCT ROWS: the CRE layers' context cross attention reads
// K / V = Wkv(Embedding(9)[label of every CRE]) (reference model_combined_modulator.py:168, layers.py:421-439), i.e. at most 9
// distinct key / value rows per head, each repeated count_c times in a gene's key sequence.  Softmax over the repeated keys is
// softmax over the distinct ones with log(count) added to the logit:
//     out = sum_c n_c exp(q . k_c) v_c / sum_c n_c exp(q . k_c)  =  sum_c softmax_c(q . k_c + log n_c) v_c
// -- the same function of (q, table, counts), N / 9 times less arithmetic and no [keys, 2D] gather of the table.  fp32 scores
// (bf16 / fp16 operands, products exact in fp32, summed in ascending d), base-2 logits (q carries scale * log2 e), weights
// normalised in fp32, output rounded once to the operand type: at least as precise as the tiled kernels, which round P to 16
// bits in front of the PV product; oracle.attention_counted restates it.  Vector arithmetic only (0.9 GFLOP per launch).
// Block = one sequence (gene) x a slab of its queries; thread = one (query, head) pair; the table lives in LDS as
// [c][d / 8][head][8] so that the 16-byte reads of the heads of a query fall on consecutive bank groups.
template <int DT, int DH>
__global__ __launch_bounds__(256) void attn_counted_keys_kernel(const unsigned short* __restrict__ q, int64_t q_stride,
                                                                const unsigned short* __restrict__ kv, int64_t kv_stride,
                                                                const float* __restrict__ log2_count, const int32_t* __restrict__ cu_q,
                                                                int C, int H, unsigned short* __restrict__ out, int64_t o_stride,
                                                                int q_per_block) {
    constexpr int NJ = DH / 8;
    extern __shared__ __attribute__((aligned(16))) char smem_ck[];
    u32x4_t* const sK = reinterpret_cast<u32x4_t*>(smem_ck);                    // [C][NJ][H] chunks of 8 values
    u32x4_t* const sV = sK + C * NJ * H;
    float* const sL = reinterpret_cast<float*>(sV + C * NJ * H);                // [C] log2 count of this sequence
    const int seq = blockIdx.y;
    const int tok0 = cu_q[seq], len = cu_q[seq + 1] - tok0;
    const int q0 = blockIdx.x * q_per_block;
    if (q0 >= len) return;
    const int D = H * DH;
    for (int i = threadIdx.x; i < 2 * C * NJ * H; i += 256) {
        const bool is_v = i >= C * NJ * H;
        const int ii = is_v ? i - C * NJ * H : i;
        const int h = ii % H, j = (ii / H) % NJ, c = ii / (H * NJ);
        (is_v ? sV : sK)[ii] = *reinterpret_cast<const u32x4_t*>(kv + (int64_t)c * kv_stride + (is_v ? D : 0) + h * DH + j * 8);
    }
    if (threadIdx.x < C) sL[threadIdx.x] = log2_count[(int64_t)seq * C + threadIdx.x];
    __syncthreads();
    const int q_end = (q0 + q_per_block < len) ? q0 + q_per_block : len;
    const int pairs = (q_end - q0) * H;
    auto unpack8 = [](u32x4_t v, float (&f)[8]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[2 * e] = Op16<DT>::to_f32((unsigned short)(v[e] & 0xffffu));
            f[2 * e + 1] = Op16<DT>::to_f32((unsigned short)(v[e] >> 16));
        }
    };
    for (int p = threadIdx.x; p < pairs; p += 256) {
        const int t = q0 + p / H, h = p % H;
        const unsigned short* qp = q + (int64_t)(tok0 + t) * q_stride + h * DH;
        float qf[DH];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float f[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(qp + 8 * j), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[8 * j + e] = f[e];
        }
        float sc[16];
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) {
            // a row this sequence does not hold is not among its keys: its K / V values -- a NaN included -- must not reach
            // the result (NaN + -inf = NaN, 0 x NaN = NaN).  Block-uniform; for finite rows the same bits as weighting by 0.
            if (sL[c] == -INFINITY) {
                sc[c] = -INFINITY;
                continue;
            }
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float f[8];
                unpack8(sK[(c * NJ + j) * H + h], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) a = __builtin_fmaf(qf[8 * j + e], f[e], a);
            }
            a += sL[c];
            sc[c] = a;
            m = __builtin_fmaxf(m, a);
        }
        float o[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) o[d] = 0.f;
        float l = 0.f;
        for (int c = 0; c < C; ++c) {
            if (sL[c] == -INFINITY) continue;
            const float pc = __builtin_amdgcn_exp2f(sc[c] - m);
            l += pc;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float f[8];
                unpack8(sV[(c * NJ + j) * H + h], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[8 * j + e] = __builtin_fmaf(pc, f[e], o[8 * j + e]);
            }
        }
        const float inv = 1.0f / l;
        unsigned short* op = out + (int64_t)(tok0 + t) * o_stride + h * DH;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u32x4_t pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = Op16<DT>::pack2(o[8 * j + 2 * e] * inv, o[8 * j + 2 * e + 1] * inv);
            *reinterpret_cast<u32x4_t*>(op + 8 * j) = pk;
        }
    }
}

template <int DT, int DH>
static int launch_counted_keys(const void* q, int64_t q_stride, const void* kv, int64_t kv_stride, const float* log2_count,
                               const int32_t* cu_q, int n_seq, int max_q, int C, int H, void* out, int64_t o_stride, hipStream_t st) {
    const int lds = 2 * C * (DH / 8) * H * 16 + C * 4;
    auto kern = attn_counted_keys_kernel<DT, DH>;
    static bool attr_set[VF_MAX_DEVICES] = {};
    const int dev = vf_current_device();
    if (dev < 0 || !attr_set[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            vf_set_error("vf_attn_counted_keys: cannot reserve LDS");
            return VF_ERR_LAUNCH;
        }
        if (dev >= 0) attr_set[dev] = true;
    }
    // a block re-reads the whole table: give it enough queries to amortise that (>= 64 per block), but enough blocks to fill
    // the chip (>= 4 per CU when the batch allows)
    int qpb = 256;
    while (qpb > 64 && (long)n_seq * ((max_q + qpb - 1) / qpb) < 1024) qpb >>= 1;
    vf_note_kernel(1, "attn_counted_keys_kernel");
    hipLaunchKernelGGL(kern, dim3((max_q + qpb - 1) / qpb, n_seq), dim3(256), lds, st, (const unsigned short*)q, q_stride,
                       (const unsigned short*)kv, kv_stride, log2_count, cu_q, C, H, (unsigned short*)out, o_stride, qpb);
    VF_CHECK_LAUNCH("vf_attn_counted_keys");
    return VF_OK;
}

extern "C" int vf_attn_counted_keys(const void* q, int64_t q_stride, const void* kv_table, int64_t kv_stride,
                                    const float* log2_count, const int32_t* cu_seqlens_q, int n_seq, int max_seqlen_q, int C,
                                    int H, int dh, void* out, int64_t o_stride, int operand_dtype, void* stream) {
    VF_REQUIRE(q && kv_table && log2_count && cu_seqlens_q && out, "vf_attn_counted_keys: null pointer");
    VF_REQUIRE(operand_dtype == VF_BF16 || operand_dtype == VF_F16, "vf_attn_counted_keys: operand_dtype must be VF_BF16 or VF_F16");
    VF_REQUIRE(C >= 1 && C <= 16 && H >= 1 && H <= 256 && (dh == 32 || dh == 48 || dh == 64),
               "vf_attn_counted_keys: C=%d (1..16) H=%d dh=%d (32 / 48 / 64) not supported", C, H, dh);
    VF_REQUIRE(2 * C * (dh / 8) * H * 16 + C * 4 <= 160 * 1024, "vf_attn_counted_keys: the key / value table does not fit the LDS");
    VF_REQUIRE(q_stride % 8 == 0 && kv_stride % 8 == 0 && o_stride % 8 == 0 && ((uintptr_t)q % 16 == 0) &&
                   ((uintptr_t)kv_table % 16 == 0) && ((uintptr_t)out % 16 == 0),
               "vf_attn_counted_keys: rows must keep 16-byte alignment");
    if (n_seq <= 0 || max_seqlen_q <= 0) return VF_OK;
    VF_REQUIRE(n_seq <= 65535, "vf_attn_counted_keys: n_seq=%d exceeds the grid limit", n_seq);
    hipStream_t st = (hipStream_t)stream;
#define VF_CK(DT_, DH_) launch_counted_keys<DT_, DH_>(q, q_stride, kv_table, kv_stride, log2_count, cu_seqlens_q, n_seq, max_seqlen_q, C, H, out, o_stride, st)
    if (operand_dtype == VF_BF16) return dh == 32 ? VF_CK(VF_BF16, 32) : dh == 48 ? VF_CK(VF_BF16, 48) : VF_CK(VF_BF16, 64);
    return dh == 32 ? VF_CK(VF_F16, 32) : dh == 48 ? VF_CK(VF_F16, 48) : VF_CK(VF_F16, 64);
#undef VF_CK
}

// Softmax over a few distinct keys with their counts, on logits a GEMM produced (vf_gemm_ln consumer with fp32 output): the
// low-rank form of the CRE layers' context cross attention.  With C <= 16 distinct key / value rows per head the logits are
// LN(x) . (Wq_h^T k_c) -- a GEMM against an [H * Cp, D] matrix built once per weights -- and the output projection of
// sum_c w_c v_c is w . (Wo_h v_c) -- a GEMM with K = H * Cp; between them only this remains:
//   w[t, h, c] = 16-bit( exp2(s[t, h, c] + log2 n[seq(t), c] - m) / sum_c' exp2(...) ),  0 for the padding slots c >= C.
// scores fp32 [tokens, >= H * Cp] (head-major, Cp slots per head), out 16-bit [tokens, >= H * Cp].  One thread per (token, head).
template <int DT>
__global__ __launch_bounds__(256) void softmax_counted_kernel(const float* __restrict__ sc, int64_t lds, const float* __restrict__ log2_count,
                                                              const int32_t* __restrict__ cu_q, int H, int Cp, int C,
                                                              unsigned short* __restrict__ out, int64_t ldo) {
    const int seq = blockIdx.y;
    const int tok0 = cu_q[seq], len = cu_q[seq + 1] - tok0;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= len * H) return;
    const int t = p / H, h = p % H;
    const float* sp = sc + (int64_t)(tok0 + t) * lds + h * Cp;
    const float* lc = log2_count + (int64_t)seq * C;
    float v[16];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        v[c] = c < C ? sp[c] + lc[c] : -INFINITY;
        m = __builtin_fmaxf(m, v[c]);
    }
    float l = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        v[c] = __builtin_amdgcn_exp2f(v[c] - m);          // exp2(-inf) = 0: absent labels and padding slots
        l += v[c];
    }
    const float inv = 1.0f / l;
    unsigned short* op = out + (int64_t)(tok0 + t) * ldo + h * Cp;
#pragma unroll
    for (int c = 0; c < 16; c += 2) {
        // the padding slots c >= C are zero whatever the row holds (0 x (1 / NaN) would make them NaN)
        const float w0 = c < C ? v[c] * inv : 0.f, w1 = c + 1 < C ? v[c + 1] * inv : 0.f;
        if (c + 1 < Cp) *reinterpret_cast<unsigned int*>(op + c) = Op16<DT>::pack2(w0, w1);
        else if (c < Cp) op[c] = (unsigned short)(Op16<DT>::pack2(w0, 0.f) & 0xffffu);
    }
}

extern "C" int vf_softmax_counted(const float* scores, int64_t lds, const float* log2_count, const int32_t* cu_seqlens_q, int n_seq,
                                  int max_seqlen_q, int H, int Cp, int C, void* out, int64_t ldo, int out_dtype, void* stream) {
    VF_REQUIRE(scores && log2_count && cu_seqlens_q && out, "vf_softmax_counted: null pointer");
    VF_REQUIRE(out_dtype == VF_BF16 || out_dtype == VF_F16, "vf_softmax_counted: out_dtype must be VF_BF16 or VF_F16");
    VF_REQUIRE(C >= 1 && C <= Cp && Cp <= 16 && Cp % 2 == 0 && H >= 1, "vf_softmax_counted: C=%d Cp=%d (C <= Cp <= 16, Cp even) H=%d", C, Cp, H);
    VF_REQUIRE(lds >= (int64_t)H * Cp && ldo >= (int64_t)H * Cp && ldo % 2 == 0 && ((uintptr_t)out % 4 == 0),
               "vf_softmax_counted: rows hold H * Cp slots; the output keeps 4-byte alignment");
    if (n_seq <= 0 || max_seqlen_q <= 0) return VF_OK;
    VF_REQUIRE(n_seq <= 65535, "vf_softmax_counted: n_seq=%d exceeds the grid limit", n_seq);
    const dim3 grid((unsigned)(((long)max_seqlen_q * H + 255) / 256), n_seq);
    if (out_dtype == VF_BF16)
        hipLaunchKernelGGL(softmax_counted_kernel<VF_BF16>, grid, dim3(256), 0, (hipStream_t)stream, scores, lds, log2_count,
                           cu_seqlens_q, H, Cp, C, (unsigned short*)out, ldo);
    else
        hipLaunchKernelGGL(softmax_counted_kernel<VF_F16>, grid, dim3(256), 0, (hipStream_t)stream, scores, lds, log2_count,
                           cu_seqlens_q, H, Cp, C, (unsigned short*)out, ldo);
    VF_CHECK_LAUNCH("vf_softmax_counted");
    return VF_OK;
}

extern "C" int vf_attn_rows_supported(int dh, int alibi, int n_seq, int H, int max_seqlen_q, int max_seqlen_k, int flags) {
    return rows_supported(dh, alibi != 0, n_seq, H, max_seqlen_q, max_seqlen_k, (flags & VF_ATTN_Q_LOG2) != 0) ? 1 : 0;
}

extern "C" int vf_attn_varlen_fwd_rows(const void* q, const void* k, const void* v, void* out, int64_t q_stride,
                                       int64_t k_stride, int64_t v_stride, int64_t o_stride, const int32_t* cu_seqlens_q,
                                       const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_q, int max_seqlen_k, int H,
                                       int dh, const float* alibi_slopes, float scale, int operand_dtype, int flags,
                                       const int64_t* q_rows, const int64_t* kv_rows, void* stream) {
    VF_REQUIRE(operand_dtype == VF_BF16 || operand_dtype == VF_F16, "vf_attn_varlen_fwd_rows: operand_dtype must be VF_BF16 or VF_F16");
    if (operand_dtype == VF_BF16)
        return attn_dispatch<VF_BF16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                      max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream, q_rows, kv_rows);
    return attn_dispatch<VF_F16>(q, k, v, out, q_stride, k_stride, v_stride, o_stride, cu_seqlens_q, cu_seqlens_k, n_seq,
                                 max_seqlen_q, max_seqlen_k, H, dh, alibi_slopes, scale, flags, stream, q_rows, kv_rows);
}

// ---------------------------------------------------------------------------------------------------------------------
// vf_attn_probs: the softmax PROBABILITIES of a few selected query rows against their sequence's keys, in fp32 -- the quantity
// the flash-style kernels above keep in registers, round to 16 bits for P . V and never write.  No V.  vf_attn_probs_v2 adds
// ALiBi (template parameter ALIBI: base-2 logit c (q . k) - log2(e) slope[h] |q_pos[r] - j|, one fma on the fp32 accumulator
// before the maximum, q_pos an explicit position per selected row) and a row map for the keys (template parameter KROWS: key j of
// sequence s is row k_rows[cu_k[s] + j] of k); the <false, false> instantiations are vf_attn_probs's kernels, instruction for
// instruction.
// Same MFMA formulation as attn_x32_kernel (v_mfma_f32_32x32x16, S^T[key 32][query 32] = K . Q^T, A = 32 key rows, B = Q^T;
// lane (query = lane & 31, hf = lane >> 5) ends up with keys (i & 3) + 8 (i >> 2) + 4 hf of ITS query in register i), but the
// fragments come straight from global memory: a few dozen rows against 10^3 keys is T * N * D MACs per sequence, two waves at
// most share a fragment (L1 serves the second), and without LDS there is no barrier an early exit could miss.
// Two passes, `stats` = (m, l) per (row, head) between them:
//   1. attn_probs_stats_kernel, wave = (sequence, 32-row tile, head): walks the keys in tiles of 32 with a running maximum m
//      (the TRUE maximum of the base-2 logits, so every exponent is <= 0 whatever the magnitude) and l = sum_j exp2(s2 - m);
//      each half wave sums its 16 keys of every tile in register order, the halves meet once at the end.
//   2. attn_probs_kernel, block = (sequence, 64-key tile, 64-row tile), wave = one 32 x 32 quadrant: loops over the heads in
//      ascending order, recomputes the logits with the same instructions on the same fragments as pass 1 (same bits),
//      P = exp2(s2 - m) / l, and either stores P per head or keeps the head sum in 16 registers and stores sum / H.
// The arithmetic of a row touches its own query, its own keys and nothing else: tile positions depend only on the row's index
// inside its sequence and on the key index, the MFMA columns (queries) and rows (keys) are independent, and no atomics: the
// bits depend neither on the rest of the call nor on max_rows / max_seqlen_k.  A NaN in a key row reaches l (and so every
// probability) of that (sequence, head) alone, one in a query row that row alone; masked columns are selected to 0 / -inf, never
// multiplied.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct ProbsParams {
    const unsigned short* q;
    const unsigned short* k;
    int64_t q_stride, k_stride;
    const int64_t* q_rows;      // selected row r's query is row q_rows[r] of q; null: row r
    const int32_t* cu_rows;     // selected rows of sequence s: [cu_rows[s], cu_rows[s + 1])
    const int32_t* cu_k;
    float c;                    // base-2 logit = c * (q . k): 1 (VF_ATTN_Q_LOG2) or scale * log2(e)
    int H, n_seq;
    int nrt;                    // 32-row tiles per sequence (pass 1)
    int max_k;
    int per_head;
    float* stats;
    float* out;
    int64_t ldo;
    const float* slopes;        // ALIBI: fp32 [H]
    const int32_t* q_pos;       // ALIBI: position of selected row r inside its key sequence; null: 0
    const int64_t* k_rows;      // KROWS: key j of sequence s is row k_rows[cu_k[s] + j] of k
};

template <int DT, int KS>
__device__ __forceinline__ void probs_load_frags(typename Op16<DT>::frag (&f)[KS], const unsigned short* p) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(p + 16 * ks);
        f[ks] = __builtin_bit_cast(typename Op16<DT>::frag, raw);
    }
}

// base-2 logits of one 32-key x 32-query tile; keys at or past `klim` (relative to the tile's first key) are -inf.
// ALIBI: slope2 = log2(e) * slope[h], dq = the lane's query position minus the tile's first key (a small integer: dq - key is
// exact); both passes go through this one function, so they add the same bias with the same two instructions.
template <int DT, int KS, bool ALIBI>
__device__ __forceinline__ void probs_logits(const typename Op16<DT>::frag (&kf)[KS], const typename Op16<DT>::frag (&qf)[KS],
                                             float c, int klim, int hf, float slope2, float dq, float (&s)[16]) {
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = Op16<DT>::mfma32(kf[ks], qf[ks], acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int key = (i & 3) + 8 * (i >> 2) + 4 * hf;
        if constexpr (ALIBI) s[i] = key < klim ? __builtin_fmaf(acc[i], c, -slope2 * __builtin_fabsf(dq - (float)key)) : -INFINITY;
        else s[i] = key < klim ? acc[i] * c : -INFINITY;
    }
}

template <int DT, int DH, bool ALIBI, bool KROWS>
__global__ __launch_bounds__(256) void attn_probs_stats_kernel(ProbsParams P) {
    using frag_t = typename Op16<DT>::frag;
    constexpr int KS = DH / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = lane & 31, hf = lane >> 5;
    const long w = (long)blockIdx.x * 4 + wave;                 // (sequence, row tile, head), head fastest; wave-uniform
    if (w >= (long)P.n_seq * P.nrt * P.H) return;
    const int h = (int)(w % P.H), rt = (int)((w / P.H) % P.nrt), seq = (int)(w / ((long)P.H * P.nrt));
    const int r0 = P.cu_rows[seq], n_rows = P.cu_rows[seq + 1] - r0;
    if (rt * 32 >= n_rows) return;
    const int k0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k0;
    const bool row_ok = rt * 32 + x < n_rows;                   // the other lanes repeat the sequence's last row and store nothing
    const int r = r0 + (row_ok ? rt * 32 + x : n_rows - 1);
    float* sp = P.stats + ((int64_t)r * P.H + h) * 2;
    if (len_k <= 0) {                                           // no keys: stats (0, 0), the row itself is zeroed by pass 2
        if (row_ok && hf == 0) { sp[0] = 0.f; sp[1] = 0.f; }
        return;
    }
    const int64_t q_row = P.q_rows ? P.q_rows[r] : (int64_t)r;
    frag_t qf[KS];
    probs_load_frags<DT, KS>(qf, P.q + q_row * P.q_stride + h * DH + 8 * hf);
    const unsigned short* kp = P.k + (KROWS ? (int64_t)0 : (int64_t)k0 * P.k_stride) + h * DH + 8 * hf;
    const float slope2 = ALIBI ? P.slopes[h] * 1.4426950408889634f : 0.f;
    const int qpos = ALIBI && P.q_pos ? P.q_pos[r] : 0;
    float m = -INFINITY, l = 0.f;
    for (int kb = 0; kb < len_k; kb += 32) {
        const int key = kb + x < len_k ? kb + x : len_k - 1;    // in bounds; the logit is masked below
        frag_t kf[KS];
        probs_load_frags<DT, KS>(kf, kp + (KROWS ? P.k_rows[k0 + key] : (int64_t)key) * P.k_stride);
        float s[16];
        probs_logits<DT, KS, ALIBI>(kf, qf, P.c, len_k - kb, hf, slope2, (float)(qpos - kb), s);
        float mx = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = max2f(mx, s[i]);
        mx = max2f(mx, __shfl_xor(mx, 32));
        const float m_new = max2f(m, mx);                       // finite from the first tile on: it holds a valid key
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += __builtin_amdgcn_exp2f(s[i] - m_new);
        l = l * __builtin_amdgcn_exp2f(m - m_new) + sum;
        m = m_new;
    }
    l += __shfl_xor(l, 32);
    if (row_ok && hf == 0) { sp[0] = m; sp[1] = l; }
}

// four consecutive columns of one output row: one 16-byte store where the row allows it (ldo is the caller's: rows are only
// 4-byte aligned in general), never past column max_k
__device__ __forceinline__ void probs_store4(float* op, int col, int max_k, f32x4_t v) {
    if (col + 3 < max_k && (reinterpret_cast<uintptr_t>(op) & 15) == 0) {
        *reinterpret_cast<f32x4_t*>(op) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < max_k) op[e] = v[e];
    }
}

template <int DT, int DH, bool ALIBI, bool KROWS>
__global__ __launch_bounds__(256) void attn_probs_kernel(ProbsParams P) {
    using frag_t = typename Op16<DT>::frag;
    constexpr int KS = DH / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = lane & 31, hf = lane >> 5;
    const int seq = blockIdx.z;
    const int r0 = P.cu_rows[seq], n_rows = P.cu_rows[seq + 1] - r0;
    const int rbase = blockIdx.y * 64 + 32 * (wave >> 1);       // this wave's quadrant: 32 rows x 32 keys; wave-uniform exits
    if (rbase >= n_rows) return;
    const int k0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k0;
    const int kbase = blockIdx.x * 64 + 32 * (wave & 1);
    if (kbase >= P.max_k) return;
    const bool row_ok = rbase + x < n_rows;
    const int r = r0 + (row_ok ? rbase + x : n_rows - 1);
    const int H = P.H;
    const int klim = len_k - kbase;                              // keys of this tile below klim exist

    if (klim <= 0) {                                             // the whole quadrant lies past the sequence's keys: zeros
        if (row_ok) {
            const int64_t n_out = P.per_head ? H : 1;
            for (int64_t o = 0; o < n_out; ++o) {
                float* op = P.out + ((int64_t)r * n_out + o) * P.ldo + kbase + 4 * hf;
#pragma unroll
                for (int g = 0; g < 4; ++g) probs_store4(op + 8 * g, kbase + 4 * hf + 8 * g, P.max_k, (f32x4_t){0.f, 0.f, 0.f, 0.f});
            }
        }
        return;
    }

    const int key = x < klim ? kbase + x : len_k - 1;
    const unsigned short* kp = P.k + (KROWS ? P.k_rows[k0 + key] : (int64_t)(k0 + key)) * P.k_stride + 8 * hf;
    const float dq = (float)((ALIBI && P.q_pos ? P.q_pos[r] : 0) - kbase);
    const int64_t q_row = P.q_rows ? P.q_rows[r] : (int64_t)r;
    const unsigned short* qp = P.q + q_row * P.q_stride + 8 * hf;
    const float* sp = P.stats + (int64_t)r * H * 2;

    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    // the next head's fragments and statistics are requested before this head's arithmetic
    frag_t kf[KS], qf[KS];
    probs_load_frags<DT, KS>(kf, kp);
    probs_load_frags<DT, KS>(qf, qp);
    float m = sp[0], l = sp[1];
    float slope = ALIBI ? P.slopes[0] : 0.f;
    for (int h = 0; h < H; ++h) {
        const int hn = h + 1 < H ? h + 1 : h;
        frag_t kn[KS], qn[KS];
        probs_load_frags<DT, KS>(kn, kp + hn * DH);
        probs_load_frags<DT, KS>(qn, qp + hn * DH);
        const float m_n = sp[2 * hn], l_n = sp[2 * hn + 1];
        const float slope_n = ALIBI ? P.slopes[hn] : 0.f;

        float s[16];
        probs_logits<DT, KS, ALIBI>(kf, qf, P.c, klim, hf, slope * 1.4426950408889634f, dq, s);
        const float inv = 1.0f / l;
        float p[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)                             // masked columns are 0 whatever m and l hold
            p[i] = ((i & 3) + 8 * (i >> 2) + 4 * hf) < klim ? __builtin_amdgcn_exp2f(s[i] - m) * inv : 0.f;
        if (P.per_head) {
            if (row_ok) {
                float* op = P.out + ((int64_t)r * H + h) * P.ldo + kbase + 4 * hf;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    probs_store4(op + 8 * g, kbase + 4 * hf + 8 * g, P.max_k, (f32x4_t){p[4 * g], p[4 * g + 1], p[4 * g + 2], p[4 * g + 3]});
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += p[i];
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { kf[ks] = kn[ks]; qf[ks] = qn[ks]; }
        m = m_n; l = l_n; slope = slope_n;
    }
    if (!P.per_head && row_ok) {
        const float inv_h = 1.0f / (float)H;
        float* op = P.out + (int64_t)r * P.ldo + kbase + 4 * hf;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            probs_store4(op + 8 * g, kbase + 4 * hf + 8 * g, P.max_k,
                         (f32x4_t){acc[4 * g] * inv_h, acc[4 * g + 1] * inv_h, acc[4 * g + 2] * inv_h, acc[4 * g + 3] * inv_h});
    }
}

template <int DT, int DH, bool ALIBI, bool KROWS>
static int launch_attn_probs(const ProbsParams& P, int max_rows, hipStream_t st) {
    const long waves = (long)P.n_seq * P.nrt * P.H;
    hipLaunchKernelGGL((attn_probs_stats_kernel<DT, DH, ALIBI, KROWS>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, P);
    VF_CHECK_LAUNCH("vf_attn_probs");
    if (P.max_k > 0) {
        hipLaunchKernelGGL((attn_probs_kernel<DT, DH, ALIBI, KROWS>), dim3((P.max_k + 63) / 64, (max_rows + 63) / 64, P.n_seq),
                           dim3(256), 0, st, P);
        VF_CHECK_LAUNCH("vf_attn_probs");
    }
    return VF_OK;
}

template <int DT, int DH>
static int launch_attn_probs_form(const ProbsParams& P, int max_rows, hipStream_t st) {
    if (P.slopes) return P.k_rows ? launch_attn_probs<DT, DH, true, true>(P, max_rows, st) : launch_attn_probs<DT, DH, true, false>(P, max_rows, st);
    return P.k_rows ? launch_attn_probs<DT, DH, false, true>(P, max_rows, st) : launch_attn_probs<DT, DH, false, false>(P, max_rows, st);
}

}  // namespace

extern "C" int vf_attn_probs_v2(const void* q, int64_t q_stride, const void* k, int64_t k_stride, const int64_t* q_rows,
                                const int32_t* cu_rows, const int32_t* cu_seqlens_k, int n_seq, int max_rows, int max_seqlen_k,
                                int H, int dh, float scale, int operand_dtype, int flags, int per_head, float* stats, float* out,
                                int64_t ldo, const float* alibi_slopes, const int32_t* q_pos, const int64_t* k_rows, void* stream) {
    const char* null_arg = !q ? "q" : !k ? "k" : !cu_rows ? "cu_rows" : !cu_seqlens_k ? "cu_seqlens_k" : !stats ? "stats" : !out ? "out" : nullptr;
    VF_REQUIRE(!null_arg, "vf_attn_probs: null pointer %s", null_arg);
    VF_REQUIRE(operand_dtype == VF_BF16 || operand_dtype == VF_F16, "vf_attn_probs: operand_dtype must be VF_BF16 or VF_F16");
    VF_REQUIRE((flags & ~VF_ATTN_Q_LOG2) == 0, "vf_attn_probs: flags 0x%x: only VF_ATTN_Q_LOG2 applies (VF_ATTN_Q_AT_START is "
               "refused: q_pos names every row's position)", flags);
    VF_REQUIRE(legacy_dh(dh), "vf_attn_probs: head_dim %d not supported (32/48/64/96/128)", dh);
    VF_REQUIRE(H > 0 && H <= 65535 && n_seq >= 0 && max_rows >= 0 && max_seqlen_k >= 0,
               "vf_attn_probs: H=%d n_seq=%d max_rows=%d max_seqlen_k=%d out of range", H, n_seq, max_rows, max_seqlen_k);
    VF_REQUIRE(ldo >= max_seqlen_k, "vf_attn_probs: ldo=%ld is below max_seqlen_k=%d", (long)ldo, max_seqlen_k);
    VF_REQUIRE(q_stride >= (int64_t)H * dh && k_stride >= (int64_t)H * dh, "vf_attn_probs: row strides must hold H * dh = %d elements", H * dh);
    VF_REQUIRE(q_stride % 8 == 0 && k_stride % 8 == 0 && ((uintptr_t)q % 16 == 0) && ((uintptr_t)k % 16 == 0) &&
                   ((uintptr_t)stats % 4 == 0) && ((uintptr_t)out % 4 == 0),
               "vf_attn_probs: q / k rows must keep 16-byte alignment");
    VF_REQUIRE(((uintptr_t)alibi_slopes % 4 == 0) && ((uintptr_t)q_pos % 4 == 0) && ((uintptr_t)k_rows % 8 == 0),
               "vf_attn_probs: alibi_slopes / q_pos / k_rows are not aligned to their element size");
    if (n_seq == 0 || max_rows == 0) return VF_OK;
    const int nrt = (max_rows + 31) / 32;
    VF_REQUIRE(n_seq <= 65535 && (max_rows + 63) / 64 <= 65535 && ((long)n_seq * nrt * H + 3) / 4 < (1L << 31),
               "vf_attn_probs: n_seq=%d max_rows=%d exceed the grid limit", n_seq, max_rows);
    ProbsParams P;
    P.q = (const unsigned short*)q; P.k = (const unsigned short*)k; P.q_stride = q_stride; P.k_stride = k_stride;
    P.q_rows = q_rows; P.cu_rows = cu_rows; P.cu_k = cu_seqlens_k;
    P.c = (flags & VF_ATTN_Q_LOG2) ? 1.0f : scale * 1.4426950408889634f;
    P.H = H; P.n_seq = n_seq; P.nrt = nrt; P.max_k = max_seqlen_k; P.per_head = per_head ? 1 : 0;
    P.stats = stats; P.out = out; P.ldo = ldo;
    P.slopes = alibi_slopes; P.q_pos = alibi_slopes ? q_pos : nullptr; P.k_rows = k_rows;
    hipStream_t st = (hipStream_t)stream;
    vf_note_kernel(1, alibi_slopes ? "attn_probs_alibi_kernel" : "attn_probs_kernel");
#define VF_PR(DT_) (dh == 32 ? launch_attn_probs_form<DT_, 32>(P, max_rows, st) : dh == 48 ? launch_attn_probs_form<DT_, 48>(P, max_rows, st) : \
                    dh == 64 ? launch_attn_probs_form<DT_, 64>(P, max_rows, st) : dh == 96 ? launch_attn_probs_form<DT_, 96>(P, max_rows, st) : \
                    launch_attn_probs_form<DT_, 128>(P, max_rows, st))
    return operand_dtype == VF_BF16 ? VF_PR(VF_BF16) : VF_PR(VF_F16);
#undef VF_PR
}

extern "C" int vf_attn_probs(const void* q, int64_t q_stride, const void* k, int64_t k_stride, const int64_t* q_rows,
                             const int32_t* cu_rows, const int32_t* cu_seqlens_k, int n_seq, int max_rows, int max_seqlen_k, int H,
                             int dh, float scale, int operand_dtype, int flags, int per_head, float* stats, float* out, int64_t ldo,
                             void* stream) {
    return vf_attn_probs_v2(q, q_stride, k, k_stride, q_rows, cu_rows, cu_seqlens_k, n_seq, max_rows, max_seqlen_k, H, dh, scale,
                            operand_dtype, flags, per_head, stats, out, ldo, nullptr, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// vf_attn_contrib (include/vf_hip_attn_contrib.h): the NORM of what key j hands to selected row r through out_proj,
//   c[r, j] = sum_h P[r, h, j] * Wo[:, h*dh:(h+1)*dh] @ v[j, h, :],   n[r, j] = ||c[r, j]||_2,
// without forming c.  With S[h, h'] = Wo_h^T Wo_h' (fp32 [H, H, dh, dh], per weights, the caller's):
//   gram kernel   G[j, h, h'] = v[j, h, :]^T S[h, h'] v[j, h', :]     one block = one head pair h <= h' (S[h, h'] staged in LDS
//                 once) walking a chunk of keys in 64-key tiles; a wave = 16 keys: T^T = S^T V_h^T on the exact fp32 MFMA
//                 (16x16x4: rows e', columns keys, k = e in ascending order), then the dot with v[j, h', :] over the
//                 accumulator registers and the four lane groups.  G[j, h', h] is the same number (S[h', h] = S[h, h']^T),
//                 stored to both places.  Consecutive blocks are the pairs of ONE key chunk, so the chunk's value rows are
//                 read from HBM once and from L2 by the other pairs.
//   norm kernel   n[r, j]^2 = sum_h P[r, h, j] * (sum_h' G[j, h, h'] P[r, h', j]), h and h' ascending, fp32 fma; one block =
//                 8 keys of one sequence (their G staged in LDS, zero padded to HT x HT) x all selected rows of the sequence.
// fp32 throughout after the 16-bit loads of v; no atomics; every (row, key) is computed by one thread from row r's P, key j's
// value row and S in a fixed order, so the bits depend neither on the rest of the call nor on max_rows / max_seqlen_k.  The
// MFMA's columns (keys) are independent: a NaN in value row (j, h) reaches G[j, h, :] and G[j, :, h] alone.  Columns past a
// sequence's keys are stored as 0, never multiplied; a negative radicand (rounding) becomes 0 through a comparison that a NaN
// fails (contrib_sqrt), so a NaN stays a NaN.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct ContribParams {
    const unsigned short* v;
    int64_t v_stride;
    const float* s_gram;
    const float* probs;
    int64_t ldp;
    const int32_t* cu_rows;
    const int32_t* cu_k;
    int n_seq, H, max_k, per_head;
    float* gram;
    float* out;
    int64_t ldo;
};

constexpr int GRAM_TILE = 64;       // keys per step of a block: 16 per wave
constexpr int GRAM_CHUNK = 512;     // keys per block
// LDS row strides in floats.  S rows: the four lane groups of an MFMA operand read rows 4s .. 4s + 3, 16 consecutive floats each:
// a stride of 16 mod 32 puts them in four different quarters of the banks.  Value rows: 16 keys x 4 consecutive floats.
template <int DH> constexpr int gram_ls() { return DH % 32 == 16 ? DH : DH + 16; }
template <int DH> constexpr int gram_vs() { return DH + 4; }
template <int DH> constexpr int gram_lds() { return 4 * (DH * gram_ls<DH>() + 2 * GRAM_TILE * gram_vs<DH>()); }

template <int DT>
__device__ __forceinline__ void gram_store8(float* dst, u32x4_t raw) {
    f32x4_t lo, hi;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        lo[2 * i] = Op16<DT>::to_f32((unsigned short)(raw[i] & 0xffffu));
        lo[2 * i + 1] = Op16<DT>::to_f32((unsigned short)(raw[i] >> 16));
        hi[2 * i] = Op16<DT>::to_f32((unsigned short)(raw[2 + i] & 0xffffu));
        hi[2 * i + 1] = Op16<DT>::to_f32((unsigned short)(raw[2 + i] >> 16));
    }
    *reinterpret_cast<f32x4_t*>(dst) = lo;
    *reinterpret_cast<f32x4_t*>(dst + 4) = hi;
}

template <int DT, int DH>
__global__ __launch_bounds__(256) void attn_contrib_gram_kernel(ContribParams P, int n_pairs) {
    extern __shared__ __attribute__((aligned(16))) float gram_smem[];
    constexpr int LS = gram_ls<DH>(), VS = gram_vs<DH>(), MT = DH / 16;
    float* S = gram_smem;
    float* Va = S + DH * LS;
    float* Vb = Va + GRAM_TILE * VS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = (int)(blockIdx.x % (unsigned)n_pairs);
    const int64_t key0 = (int64_t)(blockIdx.x / (unsigned)n_pairs) * GRAM_CHUNK;
    const int64_t total = P.cu_k[P.n_seq];
    if (key0 >= total) return;                                    // block-uniform
    const int H = P.H;
    int h = 0, rem = pair;                                        // the upper triangle, row by row
    while (rem >= H - h) { rem -= H - h; ++h; }
    const int h2 = h + rem;

    const f32x4_t* sg = reinterpret_cast<const f32x4_t*>(P.s_gram + ((int64_t)h * H + h2) * DH * DH);
    for (int c = tid; c < DH * DH / 4; c += 256)
        *reinterpret_cast<f32x4_t*>(S + (c / (DH / 4)) * LS + 4 * (c % (DH / 4))) = sg[c];

    const int kx = lane & 15, g = lane >> 4;
    const int64_t key_end = key0 + GRAM_CHUNK < total ? key0 + GRAM_CHUNK : total;
    for (int64_t t0 = key0; t0 < key_end; t0 += GRAM_TILE) {
        __syncthreads();                                          // the previous tile's operands have been read
        for (int c = tid; c < GRAM_TILE * DH / 8; c += 256) {
            const int key = c / (DH / 8), part = c % (DH / 8);
            u32x4_t ra = {0u, 0u, 0u, 0u}, rb = {0u, 0u, 0u, 0u};  // keys past the end: zeros, their results are not stored
            if (t0 + key < total) {
                const unsigned short* row = P.v + (t0 + key) * P.v_stride + 8 * part;
                ra = *reinterpret_cast<const u32x4_t*>(row + h * DH);
                rb = *reinterpret_cast<const u32x4_t*>(row + h2 * DH);
            }
            gram_store8<DT>(Va + key * VS + 8 * part, ra);
            gram_store8<DT>(Vb + key * VS + 8 * part, rb);
        }
        __syncthreads();
        const float* va = Va + (wave * 16 + kx) * VS + g;
        const float* sr = S + g * LS + kx;
        f32x4_t acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DH / 4; ++s) {
            const float b = va[4 * s];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sr[4 * s * LS + 16 * mt], b, acc[mt], 0, 0, 0);
        }
        // lane (kx, g) holds T[key kx][e' = 16 mt + 4 g + reg]
        const float* vb = Vb + (wave * 16 + kx) * VS + 4 * g;
        float dot = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4_t w = *reinterpret_cast<const f32x4_t*>(vb + 16 * mt);
#pragma unroll
            for (int e = 0; e < 4; ++e) dot = __builtin_fmaf(acc[mt][e], w[e], dot);
        }
        dot += __shfl_xor(dot, 16);
        dot += __shfl_xor(dot, 32);
        const int64_t kg = t0 + wave * 16 + kx;
        if (g == 0 && kg < total) {
            float* gp = P.gram + kg * H * H;
            gp[h * H + h2] = dot;
            gp[h2 * H + h] = dot;
        }
    }
}

// sqrt of a radicand that rounding may have pushed below zero: 0 there.  The comparison is made on the bits (negative, not -0,
// not a NaN), so it holds whatever this file's -fno-honor-nans lets the compiler assume about a float comparison (an ordered
// `x < 0` may become an unordered one, which a NaN passes; with the float form the NaN of a value row did not reach `out`):
// a NaN is not negative and stays a NaN through the square root.
__device__ __forceinline__ float contrib_sqrt(float x) {
    const unsigned u = __float_as_uint(x);
    return (u > 0x80000000u && u <= 0xff800000u) ? 0.f : __builtin_sqrtf(x);
}

template <int HT>
__global__ __launch_bounds__(256) void attn_contrib_norm_kernel(ContribParams P) {
    constexpr int KT = 8, GS = HT * HT + 4;
    __shared__ __attribute__((aligned(16))) float G[KT * GS];
    const int seq = blockIdx.y;
    const int r0 = P.cu_rows[seq], n_rows = P.cu_rows[seq + 1] - r0;
    if (n_rows <= 0) return;                                      // a sequence without selected rows writes nothing
    const int k0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k0;
    const int kbase = blockIdx.x * KT;
    const int tid = threadIdx.x, kx = tid & (KT - 1), slot = tid / KT;
    const int j = kbase + kx, H = P.H;
    if (kbase < len_k) {                                          // block-uniform; G of the tile's keys, zero padded to HT x HT
        for (int c = tid; c < KT * HT * HT; c += 256) {
            const int key = c / (HT * HT), a = (c / HT) % HT, b = c % HT;
            float x = 0.f;
            if (kbase + key < len_k && a < H && b < H) x = P.gram[(int64_t)(k0 + kbase + key) * H * H + a * H + b];
            G[key * GS + a * HT + b] = x;
        }
        __syncthreads();
    }
    if (j >= P.max_k) return;
    const float* gk = G + kx * GS;
    for (int rr = slot; rr < n_rows; rr += 256 / KT) {
        const int64_t r = r0 + rr;
        if (j >= len_k) {                                         // past the sequence's keys: zeros
            if (P.per_head) for (int h = 0; h < H; ++h) P.out[(r * H + h) * P.ldo + j] = 0.f;
            else P.out[r * P.ldo + j] = 0.f;
            continue;
        }
        float p[HT];
#pragma unroll
        for (int h = 0; h < HT; ++h) p[h] = h < H ? P.probs[(r * H + h) * P.ldp + j] : 0.f;
        if (P.per_head) {
#pragma unroll
            for (int h = 0; h < HT; ++h)
                if (h < H) {
                    P.out[(r * H + h) * P.ldo + j] = p[h] * contrib_sqrt(gk[h * HT + h]);
                }
        } else {
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < HT; ++h) {
                float t = 0.f;
#pragma unroll
                for (int q = 0; q < HT / 4; ++q) {
                    const f32x4_t w = *reinterpret_cast<const f32x4_t*>(gk + h * HT + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) t = __builtin_fmaf(w[e], p[4 * q + e], t);
                }
                acc = __builtin_fmaf(p[h], t, acc);
            }
            P.out[r * P.ldo + j] = contrib_sqrt(acc);
        }
    }
}

template <int DT, int DH>
static int launch_contrib_gram(const ContribParams& P, unsigned blocks, int n_pairs, hipStream_t st) {
    auto kern = attn_contrib_gram_kernel<DT, DH>;
    constexpr int lds = gram_lds<DH>();
    if (lds > 65536) {                             // dh >= 96: above the default dynamic-LDS limit
        static bool attr_set[VF_MAX_DEVICES] = {};
        const int dev = vf_current_device();
        if (dev < 0 || !attr_set[dev]) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
                hipSuccess) {
                (void)hipGetLastError();
                vf_set_error("vf_attn_contrib: cannot reserve %d bytes of LDS", lds);
                return VF_ERR_LAUNCH;
            }
            if (dev >= 0) attr_set[dev] = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, st, P, n_pairs);
    VF_CHECK_LAUNCH("vf_attn_contrib");
    return VF_OK;
}

template <int HT>
static int launch_contrib_norm(const ContribParams& P, hipStream_t st) {
    hipLaunchKernelGGL((attn_contrib_norm_kernel<HT>), dim3((P.max_k + 7) / 8, P.n_seq), dim3(256), 0, st, P);
    VF_CHECK_LAUNCH("vf_attn_contrib");
    return VF_OK;
}

}  // namespace

extern "C" int vf_attn_contrib(const void* v, int64_t v_stride, const float* s_gram, const float* probs, int64_t ldp,
                               const int32_t* cu_rows, const int32_t* cu_seqlens_k, int n_seq, int max_rows, int max_seqlen_k,
                               int H, int dh, int operand_dtype, int per_head, float* gram, float* out, int64_t ldo, void* stream) {
    const char* null_arg = !v ? "v" : !s_gram ? "s_gram" : !probs ? "probs" : !cu_rows ? "cu_rows" : !cu_seqlens_k ? "cu_seqlens_k"
                           : !gram ? "gram" : !out ? "out" : nullptr;
    VF_REQUIRE(!null_arg, "vf_attn_contrib: null pointer %s", null_arg);
    VF_REQUIRE(operand_dtype == VF_BF16 || operand_dtype == VF_F16, "vf_attn_contrib: operand_dtype must be VF_BF16 or VF_F16");
    VF_REQUIRE(legacy_dh(dh), "vf_attn_contrib: head_dim %d not supported (32/48/64/96/128)", dh);
    VF_REQUIRE(H > 0 && H <= 32, "vf_attn_contrib: H=%d out of range (1 .. 32: the norm kernel holds a row's H probabilities in registers)", H);
    VF_REQUIRE(n_seq >= 0 && max_rows >= 0 && max_seqlen_k >= 0,
               "vf_attn_contrib: n_seq=%d max_rows=%d max_seqlen_k=%d out of range", n_seq, max_rows, max_seqlen_k);
    VF_REQUIRE(ldo >= max_seqlen_k, "vf_attn_contrib: ldo=%ld is below max_seqlen_k=%d", (long)ldo, max_seqlen_k);
    VF_REQUIRE(ldp >= max_seqlen_k, "vf_attn_contrib: ldp=%ld is below max_seqlen_k=%d", (long)ldp, max_seqlen_k);
    VF_REQUIRE(v_stride >= (int64_t)H * dh, "vf_attn_contrib: v_stride=%ld must hold H * dh = %d elements", (long)v_stride, H * dh);
    VF_REQUIRE(v_stride % 8 == 0 && ((uintptr_t)v % 16 == 0), "vf_attn_contrib: v rows must keep 16-byte alignment (v, v_stride)");
    VF_REQUIRE(((uintptr_t)s_gram % 16 == 0) && ((uintptr_t)probs % 4 == 0) && ((uintptr_t)gram % 4 == 0) && ((uintptr_t)out % 4 == 0),
               "vf_attn_contrib: s_gram must be 16-byte aligned, probs / gram / out 4-byte aligned");
    if (n_seq == 0 || max_rows == 0) return VF_OK;
    const int n_pairs = H * (H + 1) / 2;
    const long chunks = ((long)n_seq * max_seqlen_k + GRAM_CHUNK - 1) / GRAM_CHUNK;
    VF_REQUIRE(n_seq <= 65535 && (max_rows + 63) / 64 <= 65535 && chunks * n_pairs < (1L << 31),
               "vf_attn_contrib: n_seq=%d max_rows=%d max_seqlen_k=%d exceed the grid limit", n_seq, max_rows, max_seqlen_k);
    ContribParams P;
    P.v = (const unsigned short*)v; P.v_stride = v_stride; P.s_gram = s_gram; P.probs = probs; P.ldp = ldp;
    P.cu_rows = cu_rows; P.cu_k = cu_seqlens_k; P.n_seq = n_seq; P.H = H; P.max_k = max_seqlen_k; P.per_head = per_head ? 1 : 0;
    P.gram = gram; P.out = out; P.ldo = ldo;
    hipStream_t st = (hipStream_t)stream;
    vf_note_kernel(1, "attn_contrib_kernel");
    if (max_seqlen_k == 0) return VF_OK;
    const unsigned blocks = (unsigned)(chunks * n_pairs);
#define VF_CG(DT_) (dh == 32 ? launch_contrib_gram<DT_, 32>(P, blocks, n_pairs, st) : dh == 48 ? launch_contrib_gram<DT_, 48>(P, blocks, n_pairs, st) : \
                    dh == 64 ? launch_contrib_gram<DT_, 64>(P, blocks, n_pairs, st) : dh == 96 ? launch_contrib_gram<DT_, 96>(P, blocks, n_pairs, st) : \
                    launch_contrib_gram<DT_, 128>(P, blocks, n_pairs, st))
    const int rc = operand_dtype == VF_BF16 ? VF_CG(VF_BF16) : VF_CG(VF_F16);
#undef VF_CG
    if (rc != VF_OK) return rc;
    return H <= 4 ? launch_contrib_norm<4>(P, st) : H <= 8 ? launch_contrib_norm<8>(P, st)
         : H <= 16 ? launch_contrib_norm<16>(P, st) : launch_contrib_norm<32>(P, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// vf_attn_contrib_self (include/vf_hip_gene_contrib.h): the same norms for a SELF attention with one selected row per sequence
// (the gene-body maps: the registry token over its own sequence), in the direct form.  Every key belongs to one row there, so
// a per-key Gram matrix would be shared by nobody; c[s, j, :] = sum_h P[s, h, j] * Wo_h v[t, h, :] is formed instead, a
// head-scaled GEMM [keys, H dh] x [H dh, Do] whose rows are reduced to their norms and never stored.
//   one block  = one sequence x 256 keys (8 waves x 32 keys); the keys are the MFMA's N dimension, so a lane owns ONE key (and
//                the accumulator's 16 registers are 16 rows d of c): its value fragments are 16-byte loads from the key's own
//                row (through v_rows when given), its P[s, h, j] one scalar, and no operand is shared between keys.
//   K loop     = (group of ND 32-row tiles of Wo) x (head), heads inside: the head's [32 ND, dh] slice of Wo is staged in LDS
//                once per block (register prefetch of the next slice under the MFMAs), every wave multiplies it with its keys'
//                value fragments into a ZEROED tile (dh / 16 v_mfma_f32_32x32x16: the exact fp32 product of the 16-bit
//                operands), then acc += p * tile, one v_fma_f32 per register.  After the last head the group's squares are
//                added to the key's sum in register order; after the last group the two lane halves are added and the root
//                taken.  per_head needs no acc: heads outside, groups inside, the squares of the zeroed tile summed directly.
// fp32 throughout after the 16-bit loads; no atomics; a key's arithmetic touches its own lane pair alone (the MFMA's columns
// are independent), in an order fixed by (group, head, tile, register), so the bits depend on P[s, :, j], value row t and wo
// alone.  Lanes past the sequence's keys hold zero fragments and p = 0, read nothing, and store the zeros of their columns.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct ContribSelfParams {
    const unsigned short* v;
    int64_t v_stride;
    const int64_t* v_rows;
    const unsigned short* wo;
    int64_t ldw;
    const float* probs;
    int64_t ldp;
    const int32_t* cu_k;
    int H, Do, max_k, n_tiles;
    float* out;
    int64_t ldo;
};

constexpr int CS_KEYS = 256;        // keys per block: 32 per wave
// 32-row tiles of Wo per group: the accumulators (16 registers each) and the LDS slice [32 ND, dh] set it
template <int DH> constexpr int cs_nd() { return DH <= 64 ? 8 : 4; }
// LDS row stride in elements: dh + 8 puts the 16 rows of a ds_read_b128 group in 16 different bank quads for every dh
template <int DH> constexpr int cs_ls() { return DH + 8; }

template <int DT, int DH, bool PER_HEAD>
__global__ __launch_bounds__(512) void attn_contrib_self_kernel(ContribSelfParams P) {
    using frag = typename Op16<DT>::frag;
    constexpr int ND = cs_nd<DH>(), LS = cs_ls<DH>(), KS = DH / 16, ROWS = 32 * ND, CPR = DH / 8, NCH = ROWS * CPR / 512;
    static_assert(ROWS * CPR % 512 == 0, "the Wo slice is a whole number of 16-byte chunks per thread");
    __shared__ __attribute__((aligned(16))) unsigned short W[ROWS * LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hl = lane >> 5;
    const int seq = (int)(blockIdx.x / (unsigned)P.n_tiles), tile = (int)(blockIdx.x % (unsigned)P.n_tiles);
    const int k0 = P.cu_k[seq], len_k = P.cu_k[seq + 1] - k0;
    const int H = P.H;
    const int j = tile * CS_KEYS + wave * 32 + r;
    const bool valid = j < len_k;
    if (!valid && j < P.max_k && hl == 0) {                       // past the sequence's keys: zeros
        if (PER_HEAD) for (int h = 0; h < H; ++h) P.out[((int64_t)seq * H + h) * P.ldo + j] = 0.f;
        else P.out[(int64_t)seq * P.ldo + j] = 0.f;
    }
    if (tile * CS_KEYS >= len_k) return;                          // block-uniform
    const bool wave_active = tile * CS_KEYS + wave * 32 < len_k;  // wave-uniform: a wave without keys only helps staging Wo

    const unsigned short* vp = P.v;
    if (valid) {
        const int64_t t = (int64_t)k0 + j;
        vp += (P.v_rows ? P.v_rows[t] : t) * P.v_stride + 8 * hl;
    }
    const float* pp = P.probs + (int64_t)seq * H * P.ldp + j;
    const int n_dt = P.Do / 32, NG = (n_dt + ND - 1) / ND, n_it = NG * H;

    u32x4_t wreg[NCH];
    auto load_wo = [&](int g, int h) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int q = tid + 512 * i, row = q / CPR, c = q % CPR, d = g * ROWS + row;
            wreg[i] = (u32x4_t){0u, 0u, 0u, 0u};                  // rows past Do (a partial last group): zeros, never used
            if (d < P.Do) wreg[i] = *reinterpret_cast<const u32x4_t*>(P.wo + (int64_t)d * P.ldw + h * DH + 8 * c);
        }
    };
    auto store_wo = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int q = tid + 512 * i, row = q / CPR, c = q % CPR;
            *reinterpret_cast<u32x4_t*>(W + row * LS + 8 * c) = wreg[i];
        }
    };
    auto load_v = [&](int h, u32x4_t (&dst)[KS]) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            dst[s] = (u32x4_t){0u, 0u, 0u, 0u};
            if (valid) dst[s] = *reinterpret_cast<const u32x4_t*>(vp + h * DH + 16 * s);
        }
    };
    auto it_g = [&](int it) { return PER_HEAD ? it % NG : it / H; };
    auto it_h = [&](int it) { return PER_HEAD ? it / NG : it % H; };

    u32x4_t vcur[KS], vnext[KS];
    float pcur = 0.f, pnext = 0.f;
    load_wo(it_g(0), it_h(0));
    load_v(it_h(0), vcur);
    if (valid) pcur = pp[(int64_t)it_h(0) * P.ldp];
    store_wo();
    __syncthreads();

    f32x16_t acc[ND];
    float nsq = 0.f;                                               // the key's sum of squares (PER_HEAD: of the running head)
    for (int it = 0; it < n_it; ++it) {
        const int g = it_g(it), h = it_h(it);
        const bool more = it + 1 < n_it;
        if (more) {
            const int g2 = it_g(it + 1), h2 = it_h(it + 1);
            load_wo(g2, h2);
            load_v(h2, vnext);
            pnext = valid ? pp[(int64_t)h2 * P.ldp] : 0.f;
        }
        if (wave_active) {
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                if (g * ND + dt < n_dt) {                         // block-uniform
                    f32x16_t tmp;
#pragma unroll
                    for (int i = 0; i < 16; ++i) tmp[i] = 0.f;
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const frag a = *reinterpret_cast<const frag*>(W + (dt * 32 + r) * LS + 16 * s + 8 * hl);
                        tmp = Op16<DT>::mfma32(a, __builtin_bit_cast(frag, vcur[s]), tmp);
                    }
                    if (PER_HEAD) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) nsq = __builtin_fmaf(tmp[i], tmp[i], nsq);
                    } else {
                        if (h == 0) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
                        }
#pragma unroll
                        for (int i = 0; i < 16; ++i) acc[dt][i] = __builtin_fmaf(pcur, tmp[i], acc[dt][i]);
                    }
                }
            }
            if (!PER_HEAD && h == H - 1) {
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
                    if (g * ND + dt < n_dt) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) nsq = __builtin_fmaf(acc[dt][i], acc[dt][i], nsq);
                    }
            }
            if (PER_HEAD && g == NG - 1) {
                const float tot = nsq + __shfl_xor(nsq, 32);
                if (valid && hl == 0) P.out[((int64_t)seq * H + h) * P.ldo + j] = pcur * __builtin_sqrtf(tot);
                nsq = 0.f;
            }
        }
        __syncthreads();                                          // every wave has read this slice
        if (more) store_wo();
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KS; ++s) vcur[s] = vnext[s];
        pcur = pnext;
    }
    if (!PER_HEAD && wave_active) {
        const float tot = nsq + __shfl_xor(nsq, 32);
        if (valid && hl == 0) P.out[(int64_t)seq * P.ldo + j] = __builtin_sqrtf(tot);
    }
}

template <int DT, int DH>
static int launch_contrib_self(const ContribSelfParams& P, unsigned blocks, int per_head, hipStream_t st) {
    if (per_head) hipLaunchKernelGGL((attn_contrib_self_kernel<DT, DH, true>), dim3(blocks), dim3(512), 0, st, P);
    else hipLaunchKernelGGL((attn_contrib_self_kernel<DT, DH, false>), dim3(blocks), dim3(512), 0, st, P);
    VF_CHECK_LAUNCH("vf_attn_contrib_self");
    return VF_OK;
}

}  // namespace

extern "C" int vf_attn_contrib_self(const void* v, int64_t v_stride, const int64_t* v_rows, const void* wo, int64_t ldw,
                                    const float* probs, int64_t ldp, const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_k,
                                    int H, int dh, int Do, int operand_dtype, int per_head, float* out, int64_t ldo, void* stream) {
    const char* null_arg = !v ? "v" : !wo ? "wo" : !probs ? "probs" : !cu_seqlens_k ? "cu_seqlens_k" : !out ? "out" : nullptr;
    VF_REQUIRE(!null_arg, "vf_attn_contrib_self: null pointer %s", null_arg);
    VF_REQUIRE(operand_dtype == VF_BF16 || operand_dtype == VF_F16, "vf_attn_contrib_self: operand_dtype must be VF_BF16 or VF_F16");
    VF_REQUIRE(legacy_dh(dh), "vf_attn_contrib_self: head_dim dh=%d not supported (32/48/64/96/128)", dh);
    VF_REQUIRE(Do > 0 && Do % 32 == 0, "vf_attn_contrib_self: Do=%d must be a positive multiple of 32", Do);
    VF_REQUIRE(H > 0 && H <= 1024, "vf_attn_contrib_self: H=%d out of range (1 .. 1024: H * dh is a 32-bit column offset)", H);
    VF_REQUIRE(n_seq >= 0 && max_seqlen_k >= 0, "vf_attn_contrib_self: n_seq=%d max_seqlen_k=%d out of range", n_seq, max_seqlen_k);
    VF_REQUIRE(ldo >= max_seqlen_k, "vf_attn_contrib_self: ldo=%ld is below max_seqlen_k=%d", (long)ldo, max_seqlen_k);
    VF_REQUIRE(ldp >= max_seqlen_k, "vf_attn_contrib_self: ldp=%ld is below max_seqlen_k=%d", (long)ldp, max_seqlen_k);
    VF_REQUIRE(v_stride >= (int64_t)H * dh && v_stride % 8 == 0,
               "vf_attn_contrib_self: v_stride=%ld must hold H * dh = %d elements and be a multiple of 8", (long)v_stride, H * dh);
    VF_REQUIRE(ldw >= (int64_t)H * dh && ldw % 8 == 0,
               "vf_attn_contrib_self: ldw=%ld must hold H * dh = %d elements and be a multiple of 8", (long)ldw, H * dh);
    VF_REQUIRE((uintptr_t)v % 16 == 0, "vf_attn_contrib_self: v must be 16-byte aligned");
    VF_REQUIRE((uintptr_t)wo % 16 == 0, "vf_attn_contrib_self: wo must be 16-byte aligned");
    VF_REQUIRE((uintptr_t)v_rows % 8 == 0, "vf_attn_contrib_self: v_rows must be 8-byte aligned");
    VF_REQUIRE((uintptr_t)probs % 4 == 0, "vf_attn_contrib_self: probs must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)out % 4 == 0, "vf_attn_contrib_self: out must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)cu_seqlens_k % 4 == 0, "vf_attn_contrib_self: cu_seqlens_k must be 4-byte aligned");
    const long n_tiles = ((long)max_seqlen_k + CS_KEYS - 1) / CS_KEYS;
    VF_REQUIRE((long)n_seq * n_tiles < (1L << 31),
               "vf_attn_contrib_self: n_seq=%d max_seqlen_k=%d exceed the grid limit", n_seq, max_seqlen_k);
    vf_note_kernel(1, "attn_contrib_self_kernel");
    if (n_seq == 0 || max_seqlen_k == 0) return VF_OK;
    ContribSelfParams P;
    P.v = (const unsigned short*)v; P.v_stride = v_stride; P.v_rows = v_rows; P.wo = (const unsigned short*)wo; P.ldw = ldw;
    P.probs = probs; P.ldp = ldp; P.cu_k = cu_seqlens_k; P.H = H; P.Do = Do; P.max_k = max_seqlen_k; P.n_tiles = (int)n_tiles;
    P.out = out; P.ldo = ldo;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((long)n_seq * n_tiles);
#define VF_CS(DT_) (dh == 32 ? launch_contrib_self<DT_, 32>(P, blocks, per_head, st) : dh == 48 ? launch_contrib_self<DT_, 48>(P, blocks, per_head, st) : \
                    dh == 64 ? launch_contrib_self<DT_, 64>(P, blocks, per_head, st) : dh == 96 ? launch_contrib_self<DT_, 96>(P, blocks, per_head, st) : \
                    launch_contrib_self<DT_, 128>(P, blocks, per_head, st))
    const int rc = operand_dtype == VF_BF16 ? VF_CS(VF_BF16) : VF_CS(VF_F16);
#undef VF_CS
    return rc;
}
