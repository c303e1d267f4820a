// fa_decode.hip -- KV-cache decode attention (flash-decoding) for gfx950: few query rows per
// sequence (Lq small) against a long, possibly padded K/V cache, GQA-packed and split over keys.
//
// Work item = (batch b, K/V head hkv, key split s).  Its query tile is the whole group: the
// R = G * Lq rows of the G = H / H_kv query heads that share K/V head hkv, one contiguous
// R x d block of q (packed row r = query head hkv*G + r / Lq, position i = r % Lq), so every K/V
// row is read from HBM once per group.  R <= 64, rounded up to NQB = 1, 2 or 4 blocks of 16
// MFMA columns.
//
// The four waves of a workgroup take DIFFERENT key tiles (64 keys) of the split -- wave w the
// tiles w, w + 4, ... -- each with its own (m, l, O), merged through LDS at the end: at R <= 16
// a wave per query-row block would leave three of four waves without work.
//   * S^T = K . Q^T and O^T = V^T . P^T on v_mfma_f32_16x16x32, fragment geometry of
//     fa_fwd16_kernel.hpp (key order rho, P^T straight from the accumulator into the B operand).
//   * K goes straight from HBM into VGPRs in A-operand layout (lane (g, n) loads 16 bytes of row
//     rho(n)): no wave shares a K tile with another, so LDS would only add a round trip.  The
//     next tile's K is in flight while the current one is multiplied.
//   * V goes through a two-slot LDS ring PER WAVE (LDS-DMA into the swizzled tile image of
//     fa_device.hpp, read back transposed with ds_read_b64_tr_b16); no barrier in the loop.
//   * Keys >= len_b (and, under the causal flag, the keys not every row sees) lie outside the
//     tile's buffer range: K and V rows there read as zero, never as what the cache holds, and
//     their scores are set to -inf.
//   * Causal, bottom-right aligned: only the last Lq - 1 keys of a sequence are seen by some rows
//     and not others.  Those keys never enter an MFMA (an exactly zero P times a NaN V row is
//     NaN): every wave folds its share of them into its (m, l, O) one key at a time on the VALU,
//     with masked products selected away.  All tiles below them run unmasked.
// One split: the workgroup writes O.  Several: it writes a normalised fp32 partial and a base-2
// lse (-inf for a split or row without keys) and fa_decode_combine_kernel, enqueued behind it,
// sums the splits in split order -- no counters, no workgroup waits on another.
//
// PAGED instantiations (fa_fwd_decode_paged): K / V are pools of blocks of page_size keys and key
// j of batch b is row j % page_size of block block_table[b][j / page_size].  Splits and pages are
// whole tiles, so a tile lies inside one page: its two descriptors keep their form and take their
// base from one scalar table read per tile, the entry clamped to [0, num_blocks - 1] first.  The
// tiles, their order and the arithmetic are those of the contiguous kernels (bitwise the same
// result on the gathered cache), whose code is not touched: everything paged is if constexpr.
#include <atomic>
#include <type_traits>

#include "fa_decode.hpp"
#include "fa_device.hpp"

namespace fa {

namespace {

template <typename T>
__device__ __forceinline__ float widen16(unsigned bits) {
    return (float)__builtin_bit_cast(T, (unsigned short)(bits & 0xffffu));
}

__device__ __forceinline__ float xor_max(float x, int mask) { return fmaxf(x, __shfl_xor(x, mask)); }
__device__ __forceinline__ float xor_sum(float x, int mask) { return x + __shfl_xor(x, mask); }
// 2^(a - b) as a merge weight: 0 when a is -inf, also against b = -inf
__device__ __forceinline__ float weight2(float a, float b) {
    return a == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(a - b);
}

}  // namespace

template <typename T, int D, int NQB, bool PAGED>
__global__ __launch_bounds__(kDecThreads, 1) void fa_decode_kernel(DecodeArgs a) {
    using M = Mma<T>;
    using v8 = typename M::v8;
    constexpr int ROWB = D * 2;            // bytes per tile row in LDS
    constexpr int kBK = kDecBK;
    constexpr int TILEB = kBK * ROWB;      // bytes of a V tile image
    constexpr int NKS = D / 32;            // QK^T k-steps
    constexpr int NKB = kBK / 16;          // 16-key blocks per tile
    constexpr int NDB = D / 16;            // 16-column blocks of O
    constexpr int NKK = kBK / 32;          // P.V k-steps
    constexpr int NP = TILEB / 1024;       // LDS-DMA pieces per tile
    constexpr int NVM = NKB * NKS + NP;    // VMEM operations per prefetched tile
    static_assert(D == 64 || D == 128, "decode: d = 64 or 128");
    static_assert(NVM < 64, "vmcnt range");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, g = lane >> 4;

    const int item = blockIdx.x;
    const int split = item % a.nsplit, bhk = item / a.nsplit;
    const int b = bhk / a.Hkv, hkv = bhk % a.Hkv;
    const int R = a.R, Lq = a.Lq;
    int len = a.Lk;
    if (a.seqlens) {
        const int l = a.seqlens[b];
        len = l < 0 ? 0 : l > a.Lk ? a.Lk : l;
    }
    const int kv_begin = split * a.kps;
    const int kv_end = kv_begin + a.kps < len ? kv_begin + a.kps : len;
    const bool final_ = a.nsplit == 1;
    // the group's rows in q and o; the item's partial
    const int64_t grp_off = (int64_t)bhk * R * D;
    unsigned short* const Og = (unsigned short*)a.o + grp_off;
    float* const Op = a.o_part + (int64_t)item * R * D;
    float* const Lp = a.lse + (int64_t)item * R;

    if (kv_begin >= len) {  // no key of this split exists: an empty partial (or, unsplit, zeros)
        if (final_) {
            for (int i = tid; i < R * D / 2; i += kDecThreads) ((unsigned*)Og)[i] = 0u;
        } else {
            for (int i = tid; i < R * D / 4; i += kDecThreads) ((f32x4*)Op)[i] = f32x4{};
            for (int i = tid; i < R; i += kDecThreads) Lp[i] = -INFINITY;
        }
        return;
    }

    // keys [kv_begin, mf_end) are seen by every row: the MFMA tiles.  Causal: row position i
    // sees j <= len - Lq + i, so the keys from len - Lq + 1 on go to the per-key path below.
    const int all_end = a.causal ? (len - Lq + 1 > 0 ? len - Lq + 1 : 0) : len;
    const int mf_end = kv_end < all_end ? kv_end : all_end;
    const int nt = mf_end > kv_begin ? (mf_end - kv_begin + kBK - 1) / kBK : 0;

    // Q^T fragments (B operand of QK^T): lane (g, n) holds Q[16*qb + n][32*ks + 8*g .. +7];
    // rows >= R read as zero
    const __amdgpu_buffer_rsrc_t qrs = make_rsrc((const unsigned short*)a.q + grp_off, (int64_t)R * ROWB);
    v8 qf[NQB][NKS];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            qf[qb][ks] = __builtin_bit_cast(
                v8, __builtin_amdgcn_raw_buffer_load_b128(qrs, (16 * qb + n16) * ROWB + ks * 64 + g * 16, 0, 0));

    const int krb = (int)(a.kv_stride[2] * 2);  // bytes between key rows
    // (paged: kv_stride is {block, head, row} and the bases are the head's place in block 0)
    const int64_t kv_head = (PAGED ? 0 : (int64_t)b * a.kv_stride[0]) + (int64_t)hkv * a.kv_stride[1];
    const char* const kbase = (const char*)((const unsigned short*)a.k + kv_head);
    const char* const vbase = (const char*)((const unsigned short*)a.v + kv_head);
    // Byte offset of key j's row from kbase / vbase, j wave-uniform.  Paged: one scalar read of
    // the sequence's table row (constant address space: the table is not written while the kernel
    // runs), the entry clamped into the pool before it enters an address.  Only pages that hold a
    // key of this split below len are looked up.
    typedef __attribute__((address_space(4))) const int* table_ptr;
    const table_ptr tbl = PAGED ? (table_ptr)(a.block_table + (int64_t)b * a.table_stride) : (table_ptr) nullptr;
    auto key_off = [&](int j) -> int64_t {
        if constexpr (PAGED) {
            const unsigned page = __builtin_amdgcn_readfirstlane((unsigned)j / (unsigned)a.page_size);
            const int in = j - (int)page * a.page_size;
            const int e = tbl[page];
            const int blk = e < 0 ? 0 : e > a.num_blocks - 1 ? a.num_blocks - 1 : e;
            return ((int64_t)blk * a.kv_stride[0] + (int64_t)in * a.kv_stride[2]) * 2;
        } else {
            return (int64_t)j * krb;
        }
    };

    // K fragment (A operand) of key block kb, k-step ks: row 16*kb + rho(n), bytes 64*ks + 16*g
    const int rho = 8 * ((n16 >> 2) & 1) + 4 * (n16 >> 3) + (n16 & 3);
    const int koff = rho * krb + g * 16;
    // first key of a lane's four scores inside a key block
    const int R0 = 8 * (g & 1) + 4 * (g >> 1);
    // LDS-DMA sources (the swizzled image, fa_fwd16_kernel.hpp): a 1 KiB piece lands in one group
    // of 8 rows; its lane's source chunk is XOR-swizzled by (row >> 2) & 3, whose upper bit is
    // the parity of the row group -- one source offset for even groups, one for odd ones
    int dsrc[2];
    {
        const int rem = lane * 16;
        const int r7 = (rem % 512) / 64;
#pragma unroll
        for (int odd = 0; odd < 2; ++odd) {
            const int ch = 4 * (rem / 512) + (((rem % 64) / 16) ^ ((2 * odd + (r7 >> 2)) & 3));
            dsrc[odd] = r7 * krb + ch * 16;
        }
    }
    // V^T operand reads (fa_fwd16_kernel.hpp): rows 32*kk + R0 + (n >> 2) (+16), columns 16*db + 4*(n & 3)
    char* const vring = smem + wid * 2 * TILEB;
    const int r0 = R0 + (n16 >> 2);
    const int sw = (r0 >> 2) & 3, c0 = (n16 >> 1) & 1;
    const int vrow = (r0 >> 3) * (8 * ROWB) + 64 * (r0 & 7) + 8 * (n16 & 1);
    const int vb_e = vrow + 16 * (c0 ^ sw), vb_o = vrow + 16 * ((2 + c0) ^ sw);

    f32x4 o[NDB][NQB];
    f32x4 rs[NQB];  // row sums (every register the same value)
    float m[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db][qb] = f32x4{};
        rs[qb] = f32x4{};
        m[qb] = -INFINITY;
    }
    v8 ones;
    {
        constexpr unsigned kOne = std::is_same_v<T, __bf16> ? 0x3F80u : 0x3C00u;
        ones = __builtin_bit_cast(v8, u32x4{kOne | (kOne << 16), kOne | (kOne << 16), kOne | (kOne << 16),
                                            kOne | (kOne << 16)});
    }
    const float c = a.scale_log2;

    // tile t of the split: its valid rows bound the buffer range, so rows past mf_end read as zero
    // (paged: kv_begin and the page size are multiples of the tile, so a tile lies inside one page)
    auto tile_rows = [&](int t) {
        const int left = mf_end - (kv_begin + t * kBK);
        return left < kBK ? left : kBK;
    };
    auto load_k = [&](int t, u32x4 (&kf)[NKB][NKS]) {
        const __amdgpu_buffer_rsrc_t rsr =
            make_rsrc32(kbase + key_off(kv_begin + t * kBK), (tile_rows(t) - 1) * krb + ROWB);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                kf[kb][ks] = __builtin_amdgcn_raw_buffer_load_b128(rsr, koff + kb * 16 * krb + ks * 64, 0, 0);
    };
    auto dma_v = [&](int t, char* slot) {
        const __amdgpu_buffer_rsrc_t rsr =
            make_rsrc32(vbase + key_off(kv_begin + t * kBK), (tile_rows(t) - 1) * krb + ROWB);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int rg = D == 128 ? p >> 1 : p;  // the piece's group of 8 rows (d = 128: two pieces each)
            dma16(rsr, slot + p * 1024, dsrc[rg & 1] + rg * 8 * krb + (D == 128 ? (p & 1) * 128 : 0), 0);
        }
    };

    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    auto compute = [&](int t, const u32x4 (&kf)[NKB][NKS], const char* slot) {
        f32x4 s[NKB][NQB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) {
                s[kb][qb] = f32x4{};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    s[kb][qb] = M::mma16(__builtin_bit_cast(v8, kf[kb][ks]), qf[qb][ks], s[kb][qb]);
            }
        const int nv = tile_rows(t);
        if (nv < kBK) {  // the split's last tile: keys past its end do not exist
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (16 * kb + R0 + i >= nv) {
#pragma unroll
                        for (int qb = 0; qb < NQB; ++qb) s[kb][qb][i] = -INFINITY;
                    }
        }
        u32x4 pb[NKK][NQB];  // packed P^T fragments (B operand of P.V)
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[kb][qb][i]);
            mx = xor_max(xor_max(mx, 16), 32) * c;
            // (every row sees every key of an MFMA tile and a tile has a key: m_new is finite)
            const float m_new = fmaxf(m[qb], mx);
            const float alpha = __builtin_amdgcn_exp2f(m[qb] - m_new);
            m[qb] = m_new;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    s[kb][qb][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][qb][i], c, -m_new));
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pb[kk][qb][j] = pack2<T>(s[2 * kk + (j >> 1)][qb][2 * (j & 1)], s[2 * kk + (j >> 1)][qb][2 * (j & 1) + 1]);
            rs[qb] *= alpha;
#pragma unroll
            for (int db = 0; db < NDB; ++db) o[db][qb] *= alpha;
        }
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const char* const p = slot + ((db & 1) ? vb_o : vb_e) + kk * 32 * ROWB + 512 * (db >> 1);
                const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p));
                const u32x2 hi =
                    __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * ROWB)));
                const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb)
                    o[db][qb] = M::mma16(__builtin_bit_cast(v8, vv), __builtin_bit_cast(v8, pb[kk][qb]), o[db][qb]);
            }
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) rs[qb] = M::mma16(ones, __builtin_bit_cast(v8, pb[kk][qb]), rs[qb]);
        }
    };
    // The tile in hand (K in registers, V in the LDS slot) was issued one round earlier; the next
    // one is issued before the wait, which then leaves exactly that one's NVM operations in flight.
    auto round = [&](int t, const u32x4 (&kcur)[NKB][NKS], u32x4 (&knext)[NKB][NKS], char* scur, char* snext) {
        if (t + kDecWaves < nt) {
            load_k(t + kDecWaves, knext);
            dma_v(t + kDecWaves, snext);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NVM) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        compute(t, kcur, scur);
    };

    {
        u32x4 ka[NKB][NKS], kb_[NKB][NKS];
        int t = wid;
        if (t < nt) {
            load_k(t, ka);
            dma_v(t, vring);
        }
        while (t < nt) {
            round(t, ka, kb_, vring, vring + TILEB);
            t += kDecWaves;
            if (t >= nt) break;
            round(t, kb_, ka, vring + TILEB, vring);
            t += kDecWaves;
        }
    }

    // ---- causal: the keys only some rows see, one at a time (wave w: every fourth of them)
    if (a.causal && Lq > 1) {
        const int d0 = kv_begin > all_end ? kv_begin : all_end;
        int irow[NQB];  // the row's position i, or a value that sees nothing for rows >= R
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) irow[qb] = 16 * qb + n16 < R ? (16 * qb + n16) % Lq : -(1 << 30);
        for (int j = d0 + wid; j < kv_end; j += kDecWaves) {
            const int64_t joff = key_off(j);  // (paged: these keys may straddle a page boundary)
            const char* const kr = kbase + joff;
            const char* const vr = vbase + joff;
            u32x4 kq[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) kq[ks] = *(const u32x4*)(kr + ks * 64 + g * 16);
            u32x2 vq[NDB];
#pragma unroll
            for (int db = 0; db < NDB; ++db) vq[db] = *(const u32x2*)(vr + 32 * db + 8 * g);
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) {
                float dot = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const u32x4 qq = __builtin_bit_cast(u32x4, qf[qb][ks]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        dot = __builtin_fmaf(widen16<T>(qq[e]), widen16<T>(kq[ks][e]), dot);
                        dot = __builtin_fmaf(widen16<T>(qq[e] >> 16), widen16<T>(kq[ks][e] >> 16), dot);
                    }
                }
                dot = xor_sum(xor_sum(dot, 16), 32);
                const bool vis = j <= len - Lq + irow[qb];
                const float sc = vis ? dot * c : -INFINITY;
                const float m_new = fmaxf(m[qb], sc);
                const float alpha = weight2(m[qb], m_new);
                const float p = vis ? __builtin_amdgcn_exp2f(sc - m_new) : 0.f;
                m[qb] = m_new;
                rs[qb] = rs[qb] * alpha + p;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    f32x4 vf;
                    vf[0] = widen16<T>(vq[db][0]);
                    vf[1] = widen16<T>(vq[db][0] >> 16);
                    vf[2] = widen16<T>(vq[db][1]);
                    vf[3] = widen16<T>(vq[db][1] >> 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[db][qb][e] = o[db][qb][e] * alpha + (vis ? p * vf[e] : 0.f);
                }
            }
        }
    }

    // ---- merge the waves' states: waves 1..3 leave theirs in LDS lane by lane (the rings are
    // idle behind the barrier), wave 0 folds them in wave order
    constexpr int NREG = NDB * NQB * 4 + 2 * NQB;
    static_assert((kDecWaves - 1) * NREG * 64 * 4 <= decode_lds_bytes(D), "merge area fits the rings");
    float* const xs = (float*)smem;
    __syncthreads();
    if (wid > 0) {
        float* const x = xs + (wid - 1) * NREG * 64 + lane;
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            x[(2 * qb) * 64] = m[qb];
            x[(2 * qb + 1) * 64] = rs[qb][0];
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int e = 0; e < 4; ++e) x[(2 * NQB + (qb * NDB + db) * 4 + e) * 64] = o[db][qb][e];
        }
    }
    __syncthreads();
    if (wid > 0) return;
    float l[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) l[qb] = rs[qb][0];
    for (int w2 = 0; w2 < kDecWaves - 1; ++w2) {
        const float* const x = xs + w2 * NREG * 64 + lane;
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            const float m2 = x[(2 * qb) * 64], l2 = x[(2 * qb + 1) * 64];
            const float m_new = fmaxf(m[qb], m2);
            const float w1 = weight2(m[qb], m_new), wg2 = weight2(m2, m_new);
            m[qb] = m_new;
            l[qb] = l[qb] * w1 + l2 * wg2;
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[db][qb][e] = o[db][qb][e] * w1 + x[(2 * NQB + (qb * NDB + db) * 4 + e) * 64] * wg2;
        }
    }

    // ---- lane (g, n) holds O^T[16*db + 4*g + e][row 16*qb + n]; a row without keys gives zeros
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        const int r = 16 * qb + n16;
        if (r >= R) continue;
        const float inv = l[qb] > 0.f ? 1.f / l[qb] : 0.f;
        if (final_) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const f32x4 x = o[db][qb] * inv;
                *(u32x2*)(Og + r * D + 16 * db + 4 * g) = u32x2{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3])};
            }
        } else {
#pragma unroll
            for (int db = 0; db < NDB; ++db) *(f32x4*)(Op + r * D + 16 * db + 4 * g) = o[db][qb] * inv;
            // lse in log2 units: m + log2(l)  (v_log_f32 is log2)
            if (g == 0) Lp[r] = l[qb] > 0.f ? m[qb] + __builtin_amdgcn_logf(l[qb]) : -INFINITY;
        }
    }
}

// O = sum_s 2^(lse_s - M) O_s / sum_s 2^(lse_s - M), M = max_s lse_s, in split order; splits
// without keys (lse = -inf) weigh nothing and a row with none at all is zero.  One thread per
// (b, hkv, packed row, four columns).
template <typename T, int D>
__global__ __launch_bounds__(256) void fa_decode_combine_kernel(DecodeArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)a.B * a.Hkv * a.R * (D / 4);
    if (idx >= total) return;
    const int c4 = (int)(idx % (D / 4));
    const int64_t row = idx / (D / 4);  // bhk * R + r
    const int r = (int)(row % a.R);
    const int64_t bhk = row / a.R;
    const int ns = a.nsplit;
    const float* const lp = a.lse + bhk * ns * a.R + r;
    const float* const op = a.o_part + (bhk * ns * a.R + r) * D + 4 * c4;
    float Mx = -INFINITY;
    for (int s = 0; s < ns; ++s) Mx = fmaxf(Mx, lp[(int64_t)s * a.R]);
    f32x4 acc = f32x4{};
    float wsum = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float wgt = weight2(lp[(int64_t)s * a.R], Mx);
        acc += wgt * *(const f32x4*)(op + (int64_t)s * a.R * D);
        wsum += wgt;
    }
    const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
    acc *= inv;
    *(u32x2*)((unsigned short*)a.o + row * D + 4 * c4) = u32x2{pack2<T>(acc[0], acc[1]), pack2<T>(acc[2], acc[3])};
}

template <typename T, int D, int NQB, bool PAGED>
static hipError_t launch_decode_one(const DecodeArgs& a, hipStream_t s) {
    static const char* const names[2][3] = {
        {"fa_decode_kernel<16 rows>", "fa_decode_kernel<32 rows>", "fa_decode_kernel<64 rows>"},
        {"fa_decode_kernel<16 rows, paged>", "fa_decode_kernel<32 rows, paged>", "fa_decode_kernel<64 rows, paged>"}};
    constexpr int lds = decode_lds_bytes(D);
    // (more than 64 KiB of dynamic LDS at d = 128: raise the kernel's limit once per device.  The
    // attribute is set on the device that is current at the call -- the stream's, by the header's
    // contract -- so that is the device remembered; one that cannot be told is set on every launch)
    static std::atomic<unsigned long long> raised{0};
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        dev = -1;
    }
    if (dev < 0 || !(raised.load(std::memory_order_relaxed) >> dev & 1)) {
        if (hipFuncSetAttribute((const void*)fa_decode_kernel<T, D, NQB, PAGED>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            (void)hipGetLastError();
        else if (dev >= 0)
            raised.fetch_or(1ull << dev, std::memory_order_relaxed);
    }
    const int64_t grid = (int64_t)a.B * a.Hkv * a.nsplit;
    note_kernel(names[PAGED][NQB == 1 ? 0 : NQB == 2 ? 1 : 2], grid);
    hipLaunchKernelGGL((fa_decode_kernel<T, D, NQB, PAGED>), dim3((unsigned)grid), dim3(kDecThreads), lds, s, a);
    if (hipError_t he = hipGetLastError()) return he;
    if (a.nsplit > 1) {
        const int64_t cgrid = ((int64_t)a.B * a.Hkv * a.R * (D / 4) + 255) / 256;
        note_kernel("fa_decode_combine_kernel", cgrid);
        hipLaunchKernelGGL((fa_decode_combine_kernel<T, D>), dim3((unsigned)cgrid), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <typename T, int D, bool PAGED>
static hipError_t launch_decode_r(const DecodeArgs& a, hipStream_t s) {
    if (a.R <= 16) return launch_decode_one<T, D, 1, PAGED>(a, s);
    if (a.R <= 32) return launch_decode_one<T, D, 2, PAGED>(a, s);
    return launch_decode_one<T, D, 4, PAGED>(a, s);
}

template <typename T, bool PAGED>
static hipError_t launch_decode_d(int d, const DecodeArgs& a, hipStream_t s) {
    if (d == 64) return launch_decode_r<T, 64, PAGED>(a, s);
    if (d == 128) return launch_decode_r<T, 128, PAGED>(a, s);
    return hipErrorInvalidValue;
}

template <typename T>
static hipError_t launch_decode_t(int d, const DecodeArgs& a, hipStream_t s) {
    return a.block_table ? launch_decode_d<T, true>(d, a, s) : launch_decode_d<T, false>(d, a, s);
}

hipError_t launch_decode(Elem t, int d, const DecodeArgs& a, hipStream_t s) {
    if (a.R < 1 || a.R > kDecMaxRows || a.nsplit < 1 || a.kps % kDecBK || (a.nsplit > 1 && (!a.o_part || !a.lse)))
        return hipErrorInvalidValue;
    // paged: whole tiles per page (a tile's descriptor never straddles two blocks), a pool to clamp into
    if (a.block_table && (a.page_size <= 0 || a.page_size % kDecBK || a.num_blocks <= 0 || a.table_stride <= 0))
        return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_decode_t<__bf16>(d, a, s);
    if (t == Elem::F16) return launch_decode_t<_Float16>(d, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
