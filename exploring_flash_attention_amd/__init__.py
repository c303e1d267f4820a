"""exploring_flash_attention_amd -- MI355X (gfx950)-native flash-attention forward.

Drop-in for the attention-forward path of tyler-utah/exploring_flash_attention: the same
``Q, K, V -> O`` call surfaces (``v1``, ``tiled_d``, ``v2`` modules mirror the reference's
flash_attention_v1 / flash_attention_v1_tiled_d / flash_attention_v2 families), backed by
hand-written CDNA4 HIP kernels behind a C ABI (include/fa_mi355x.h,
``_lib/libfa_mi355x.so``).  ``ops`` has the zero-copy device-tensor operators and
``dist`` the split-KV forward sharded over the GPUs of a node with RCCL.
``attention_v1`` / ``flash_attention_v1`` take ``causal=True`` (row i attends to keys 0..i;
bf16 / fp16, d <= 256) and grouped-query K / V (``[B, H_kv, L, d]`` with H a multiple of H_kv;
same types and head dims); ``attention_decode`` is the KV-cache decode forward (few query rows
against a long, padded cache: ``[B, H, Lq, d]`` x ``[B, H_kv, Lk, d]``, per-sequence key
lengths, bottom-right causal mask, GQA-packed and split over keys; bf16 / fp16, d <= 128) and
``attention_decode_paged`` the same forward on a paged pool ``[num_blocks, page_size, H_kv, d]``
read in place through an int32 block table (page_size a multiple of 64, d = 64 / 128);
``attention_varlen`` is the prefill forward of a ragged batch: token-packed ``[T, H, d]`` q and
``[T, H_kv, d]`` k / v with a device-side int32 ``cu_seqlens``, one launch, no padding, causal
or not (bf16 / fp16, d <= 256), a slice of a fused QKV projection read in place;
``attention_varlen_paged`` is that forward with the keys in the paged pool (chunked prefill against
the cache ``attention_decode_paged`` reads, no gather) and ``kv_cache_append_paged`` writes a
chunk's new K / V into the pool's pages;
every other surface is non-causal with H_kv = H and Lq = Lk, as the reference is.

There is no CPU fallback: every entry point raises if the HIP library is not built or no
ROCm device is present.
"""
from . import ops  # noqa: F401
from .ops import (attention_decode, attention_decode_paged, attention_partial, attention_tiled_d,  # noqa: F401
                  attention_v1, attention_v2, attention_varlen, attention_varlen_paged, combine,
                  kernel_geometry, kv_cache_append_paged)
from .tiled_d import flash_attention_v1_tiled_d  # noqa: F401
from .v1 import flash_attention_v1  # noqa: F401
from .v2 import flash_attention_v2  # noqa: F401

__all__ = ["ops", "attention_v1", "attention_tiled_d", "attention_v2", "attention_partial",
           "attention_decode", "attention_decode_paged", "attention_varlen", "attention_varlen_paged",
           "kv_cache_append_paged",
           "combine", "kernel_geometry", "flash_attention_v1", "flash_attention_v1_tiled_d",
           "flash_attention_v2"]
__version__ = "0.1.0"
