// fa_kv_append.hip -- a prefill chunk's new K / V rows into the pages of a paged KV cache
// (fa_kv_append_paged): k_new / v_new are token-packed [T, H_kv, d] (strides {token, head}), the
// pools [num_blocks, page_size, H_kv, d] (strides {block, head, row}) and the block table, the
// sequence offsets and the key counts int32 arrays on the device; nothing is read on the host.
//
// Sequence b owns token rows [start, start + len_q) of k_new / v_new, clamped exactly as the varlen
// forward clamps its query side: start = clamp(cu[b], 0, T), len_q = clamp(cu[b+1] - start, 0,
// min(max_seqlen, T - start)).  seqused_k[b] is its key count AFTER the append -- the array the
// attention call then takes -- so new token i is logical key p = seqused_k[b] - len_q + i and goes
// to row p % page_size of block clamp(block_table[b][p / page_size], 0, num_blocks - 1).  A token
// with p < 0 or p >= max_seqlen_k (the keys the table maps) cannot be placed and is skipped.
//
// Plain data movement: a work item is (sequence, block of kAppendRows token rows, K/V head), a
// thread moves 16 bytes of K and 16 of V at a time with vector loads and stores.  No LDS, no DMA,
// no atomics.  Bounds: a source row is st + i < T; a destination is a row below page_size of a
// block below num_blocks at a head below H_kv, and only table entries below ceil(max_seqlen_k /
// page_size) <= table_stride are read.  Rows that no token owns are never written.
#include "fa_device.hpp"

namespace fa {

__global__ __launch_bounds__(kAppendThreads) void fa_kv_append_kernel(AppendArgs a) {
    const unsigned item = blockIdx.x;
    const unsigned hkv = item % (unsigned)a.Hkv, rest = item / (unsigned)a.Hkv;
    const unsigned rb = rest % (unsigned)a.nrb, b = rest / (unsigned)a.nrb;
    const int64_t nt = a.total_rows;
    const int64_t c0 = a.cu_seqlens[b], c1 = a.cu_seqlens[b + 1];
    const int64_t st = c0 < 0 ? 0 : c0 > nt ? nt : c0;
    const int64_t room = nt - st < a.max_seqlen ? nt - st : a.max_seqlen;
    const int64_t n = c1 - st;
    const int len_q = (int)(n < 0 ? 0 : n > room ? room : n);
    const int row0 = (int)rb * kAppendRows;
    if (row0 >= len_q) return;  // past the sequence's end
    const int64_t p0 = (int64_t)a.seqused_k[b] - len_q;  // logical key of the sequence's new token 0
    const int* const tbl = a.block_table + (int64_t)b * a.table_stride;
    const unsigned short* const kn = (const unsigned short*)a.k_new + (int64_t)hkv * a.new_stride[1];
    const unsigned short* const vn = (const unsigned short*)a.v_new + (int64_t)hkv * a.new_stride[1];
    unsigned short* const kc = (unsigned short*)a.k_cache + (int64_t)hkv * a.cache_stride[1];
    unsigned short* const vc = (unsigned short*)a.v_cache + (int64_t)hkv * a.cache_stride[1];
    const int rows = len_q - row0 < kAppendRows ? len_q - row0 : kAppendRows;
    for (int idx = threadIdx.x; idx < rows * a.chunks; idx += kAppendThreads) {
        const int r = idx / a.chunks, c = idx - r * a.chunks;
        const int i = row0 + r;
        const int64_t p = p0 + i;
        if (p < 0 || p >= a.max_seqlen_k) continue;  // no page for this key
        const int page = (int)(p / a.page_size), in = (int)(p - (int64_t)page * a.page_size);
        const int e = tbl[page];
        const int blk = e < 0 ? 0 : e > a.num_blocks - 1 ? a.num_blocks - 1 : e;
        const int64_t src = (st + i) * a.new_stride[0] + c * 8;
        const int64_t dst = (int64_t)blk * a.cache_stride[0] + (int64_t)in * a.cache_stride[2] + c * 8;
        const u32x4 kk = *(const u32x4*)(kn + src);
        const u32x4 vv = *(const u32x4*)(vn + src);
        *(u32x4*)(kc + dst) = kk;
        *(u32x4*)(vc + dst) = vv;
    }
}

hipError_t launch_kv_append(const AppendArgs& a, hipStream_t s) {
    if (!a.k_new || !a.v_new || !a.k_cache || !a.v_cache || !a.cu_seqlens || !a.seqused_k || !a.block_table ||
        a.B <= 0 || a.nrb <= 0 || a.Hkv <= 0 || a.chunks <= 0 || a.chunks > 32 || a.max_seqlen <= 0 ||
        a.total_rows <= 0 || a.page_size <= 0 || a.num_blocks <= 0 || a.max_seqlen_k <= 0 ||
        a.table_stride < (a.max_seqlen_k + a.page_size - 1) / a.page_size)
        return hipErrorInvalidValue;
    const int64_t grid = (int64_t)a.B * a.nrb * a.Hkv;
    if (grid >= (int64_t)1 << 31) return hipErrorInvalidValue;
    note_kernel("fa_kv_append_kernel", grid);
    hipLaunchKernelGGL(fa_kv_append_kernel, dim3((unsigned)grid), dim3(kAppendThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fa
