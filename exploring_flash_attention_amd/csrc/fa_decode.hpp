// fa_decode.hpp -- shared between the KV-cache decode kernels (fa_decode.hip) and the C-ABI
// layer (fa_capi.cpp): the arguments, the geometry the planner needs, the launcher.
#pragma once
#include "fa_internal.hpp"

namespace fa {

constexpr int kDecBK = 64;       // keys per tile (one wave's unit of work)
constexpr int kDecWaves = 4;     // waves per workgroup, each on its own key tiles of the split
constexpr int kDecThreads = kDecWaves * 64;
constexpr int kDecMaxRows = 64;  // packed query rows R = G * Lq per work item at most
// keys a split should keep at least, so that every wave of its workgroup has a tile
constexpr int kDecMinSplitKeys = kDecWaves * kDecBK;
// LDS: a two-slot V ring per wave (the partial-state exchange at the end reuses it)
constexpr int decode_lds_bytes(int d) { return kDecWaves * 2 * kDecBK * d * 2; }
// workgroups per CU the planner counts on (LDS-bound: 128 KiB at d = 128, 64 KiB at d = 64)
constexpr int decode_wg_per_cu(int) { return 1; }

// One work item = (batch b, K/V head hkv, key split s), item index (b * Hkv + hkv) * nsplit + s.
struct DecodeArgs {
    const void* q;        // [B][H][Lq][D] contiguous: the group's R = G * Lq rows are one block
    const void* k;        // [B][Hkv][Lk][D] through kv_stride (elements; d contiguous)
    const void* v;
    void* o;              // [B][H][Lq][D] contiguous
    const int* seqlens;   // [B] or null: keys >= clamp(seqlens[b], 0, Lk) do not exist
    int B, H, Hkv, G, Lq, Lk;
    int R;                // G * Lq
    int nsplit;           // key splits per (b, hkv)
    int kps;              // keys per split, a multiple of kDecBK
    int causal;           // bottom-right aligned: row position i sees keys j <= len - Lq + i
    int64_t kv_stride[3]; // {batch, head, row}
    float scale_log2;     // log2(e) * softmax_scale
    // nsplit > 1: normalised fp32 partial O [item][R][D] and base-2 lse [item][R] (-inf: empty)
    float* o_part;
    float* lse;
    // paged cache (block_table != null): k / v are pools of num_blocks blocks of page_size keys,
    // kv_stride is {block, head, row} and key j of batch b lives in block
    // clamp(block_table[b * table_stride + j / page_size], 0, num_blocks - 1), row j % page_size
    const int* block_table;
    int64_t table_stride;
    int page_size;        // a multiple of kDecBK: a tile never straddles two pages
    int num_blocks;
};

// (a.block_table selects the paged kernels)
hipError_t launch_decode(Elem t, int d, const DecodeArgs& a, hipStream_t s);

}  // namespace fa
