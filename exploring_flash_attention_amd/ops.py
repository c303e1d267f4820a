"""Device-tensor operators over the C ABI (torch tensors in HBM, zero-copy).

Every function takes ``[B, H, L, d]`` bf16 / fp16 (or fp64) tensors on a ROCm device --
contiguous, or for attention_v1 / _tiled_d / _v2 any view with a contiguous d (strided
kernels, no copy) --
launches on the current HIP stream of that device and returns without synchronising.
PyTorch is only the plumbing here (device memory, streams); the work is done by the
gfx950 kernels in libfa_mi355x.so.

Reference launchers these replace (tyler-utah/exploring_flash_attention):
  attention_v1       flash_attention_v1/CUDA/flash_attention_v1.h:251 (opt1 :354)
  attention_tiled_d  flash_attention_v1_tiled_d/CUDA/flash_attention_v1.h:312 (opt :448)
  attention_v2       flash_attention_v2/CUDA/flash_attention_v2.h:438 (opt :559)
  attention_partial  partial_attention_kernel, flash_attention_v2/CUDA/flash_attention_v2.h:243
  combine            reduction_kernel,         flash_attention_v2/CUDA/flash_attention_v2.h:356
attention_decode (KV-cache decode: Lq != Lk, per-sequence key lengths, GQA-packed split-KV),
attention_decode_paged (the same on a paged pool, through a block table), attention_varlen
(ragged prefill batches: token-packed [T, H, d] tensors with a device-side cu_seqlens),
attention_varlen_paged (that prefill with the keys in the paged pool) and kv_cache_append_paged
(a chunk's new K / V into the pool's pages) have no counterpart in the reference.
"""
import contextlib
import ctypes
import functools
import threading

import torch

from . import _lib
from ._lib import (FA_BLOCKS_PER_WG_AUTO, FA_DTYPE_BF16, FA_DTYPE_FP16, FA_DTYPE_FP16_SCALED, FA_DTYPE_FP32,
                   FA_DTYPE_FP64, FA_KV_TILES_AUTO, check, lib)

# torch.float64 runs the fp64 kernels (the reference's USE_FP64 build): fp64 MFMA, softmax,
# partials and lse -- the bit-tight mode, not the fast one
_DTYPES = {torch.bfloat16: FA_DTYPE_BF16, torch.float16: FA_DTYPE_FP16, torch.float64: FA_DTYPE_FP64}
# split-KV partial formats: a torch dtype, or PARTIAL_FP16_SCALED (fp16 scaled per row by a
# power of two, exponent beside the lse: half the bytes of fp32, attention_v2 only)
PARTIAL_FP16_SCALED = "fp16_scaled"
_PDTYPES = {torch.float32: FA_DTYPE_FP32, torch.bfloat16: FA_DTYPE_BF16, torch.float16: FA_DTYPE_FP16,
            torch.float64: FA_DTYPE_FP64, PARTIAL_FP16_SCALED: FA_DTYPE_FP16_SCALED}


_klog = threading.local()


def _launched(status):
    """check() for a call that launches kernels; inside launched_kernels() also records what
    the library's launcher enqueued (fa_last_kernels)."""
    check(status)
    log = getattr(_klog, "log", None)
    if log is not None:
        log.append(_lib.last_kernels())


@contextlib.contextmanager
def launched_kernels():
    """Collect, in call order, the kernels (with grids) every operator of this module launches
    on this thread inside the block -- the library's own report (fa_last_kernels), so a caller
    such as bench.py names what ran instead of restating the launch rules."""
    prev = getattr(_klog, "log", None)
    _klog.log = []
    try:
        yield _klog.log
    finally:
        _klog.log = prev


def _default_pdtype(dtype, partial_dtype, fused=False):
    """Partial format when none is given: fp64 for fp64 inputs; the fused split-KV
    (attention_v2) keeps per-row scaled fp16 partials -- half the workspace traffic of fp32
    at C4 (4.73 -> 3.50 ms) and within a few output ulps of it (tests/test_gpu.py); the
    row-layout partials of the multi-GPU path stay fp32."""
    if partial_dtype is not None:
        return partial_dtype
    if dtype == torch.float64:
        return torch.float64
    return PARTIAL_FP16_SCALED if fused else torch.float32

SUPPORTED_HEAD_DIMS = (32, 64, 128, 256, 384, 512)  # head dims with a kernel
# head dims past one LDS tile: the d-tiled kernels (csrc/fa_fwd_dtiled.hip), contiguous tensors,
# FA-v1 / tiled-d / unsplit v2 only (no split-KV partial kernel, no multi-GPU path)
WIDE_HEAD_DIMS = (384, 512)
MAX_HEAD_DIM = 512


def kernel_head_dim(d):
    """Head dim of the kernel that serves head dim d: d itself when a kernel exists,
    otherwise the next larger one (the operators then zero-pad q, k, v to it and keep the
    softmax scale 1/sqrt(d); zero columns add nothing to q k^T and come out of P.V as zeros).
    The reference's Python functions take any d, e.g. d = 16 in its tests' shapes."""
    d = int(d)
    if d <= 0 or d > MAX_HEAD_DIM:
        raise ValueError(f"head dim d={d} unsupported (1 <= d <= {MAX_HEAD_DIM})")
    return next(D for D in SUPPORTED_HEAD_DIMS if D >= d)


def _pad_d(t, D):
    return t if t.shape[-1] == D else torch.nn.functional.pad(t, (0, D - t.shape[-1])).contiguous()


def _unpad_into(o_pad, o, d):
    if o_pad is not o:
        o.copy_(o_pad[..., :d])
    return o


def _on_tensor_device(fn):
    """Run a launching operator with the device of its first tensor current.  The stream handed
    to the library is that device's current stream, but the default stream's handle is 0 on every
    device and the runtime resolves it -- and the occupancy plans, the counter reset and torch's
    temporaries -- to the CURRENT device: without the guard a call on cuda:1 tensors while cuda:0
    is current would enqueue on cuda:0.  The caller's current device is restored on return."""
    first = fn.__code__.co_varnames[0]

    @functools.wraps(fn)
    def guarded(*args, **kw):
        t = args[0] if args else kw.get(first)
        if isinstance(t, torch.Tensor) and t.is_cuda:
            with torch.cuda.device(t.device):
                return fn(*args, **kw)
        return fn(*args, **kw)  # not a device tensor: the operator's own checks name it
    return guarded


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stride_args(q, k, v, o):
    """Stride arguments of the *_ex entry points for a mix of contiguous and strided
    [B, H, L, d] tensors: None when all four are contiguous, False when some view is not
    expressible (d not contiguous, strides not multiples of 8 elements, k and v strided
    differently, fp64), else three ctypes int64[3] arrays {batch, head, row} for q, k/v, o."""
    ts = (q, k, v, o)
    if all(t.is_contiguous() for t in ts):
        return None
    if q.dtype not in (torch.bfloat16, torch.float16) or k.stride() != v.stride():
        return False

    def ok(t):
        st = t.stride()
        return (st[3] == 1 and all(x > 0 and x % 8 == 0 for x in st[:3]) and st[2] >= t.shape[3]
                and t.data_ptr() % 16 == 0)

    if not all(ok(t) for t in ts):
        return False
    return tuple((ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (q, k, o))


def _via_contiguous(fn, q, k, v, o, **kw):
    """Run fn on contiguous copies of views the strided kernels cannot address."""
    o.copy_(fn(q.contiguous(), k.contiguous(), v.contiguous(), **kw))
    return o


def _check_tensor(name, t, dtype=None, device=None, ndim=4, strided=False):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a ROCm device tensor (got device {t.device}); "
                         "the MI355X path has no CPU fallback")
    if t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if not strided and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")


def _check_qkv(q, k, v, same_len=True, strided=False, gqa=False):
    """The common q / k / v checks.  gqa: k and v may hold H_kv heads with H % H_kv == 0
    (attention_v1 only); returns the group size G = H / H_kv (1 everywhere else)."""
    _check_tensor("q", q, strided=strided)
    if q.dtype not in _DTYPES:
        raise ValueError(f"q dtype {q.dtype} unsupported (bfloat16, float16 or float64)")
    _check_tensor("k", k, q.dtype, q.device, strided=strided)
    _check_tensor("v", v, q.dtype, q.device, strided=strided)
    if k.shape != v.shape:
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} must have the same shape")
    if q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on B, H or d")
    H, Hkv = q.shape[1], k.shape[1]
    if H != Hkv:
        if not gqa:
            raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on B, H or d "
                             "(grouped-query attention, H_kv < H, is served by attention_v1 only)")
        if Hkv <= 0 or H % Hkv:
            raise ValueError(f"grouped-query attention: H={H} query heads are not a multiple of "
                             f"H_kv={Hkv} K/V heads")
    if same_len and (q.shape[0], q.shape[2], q.shape[3]) != (k.shape[0], k.shape[2], k.shape[3]):
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} must have the same shape")
    return H // Hkv if H != Hkv else 1


def _out(out, q, shape=None, dtype=None, strided=False):
    shape = tuple(q.shape) if shape is None else shape
    dtype = q.dtype if dtype is None else dtype
    if out is None:
        return torch.empty(shape, dtype=dtype, device=q.device)
    _check_tensor("out", out, dtype, q.device, ndim=len(shape), strided=strided)
    if tuple(out.shape) != shape:
        raise ValueError(f"out has shape {tuple(out.shape)}, expected {shape}")
    return out


def _attention_v1_causal(q, k, v, o):
    """attention_v1(causal=True) after the common checks: fa_fwd_v1_causal on contiguous
    tensors of a kernel head dim, zero-padded or copied to that form otherwise."""
    B, H, L, d = q.shape
    if q.dtype == torch.float64:
        raise NotImplementedError("causal attention: float64 tensors are not supported (the fp64 kernels "
                                  "have no causal mode; use bfloat16 or float16)")
    if d > 256:
        raise NotImplementedError(f"causal attention: head dim d={d} is not supported (1 <= d <= 256; the "
                                  "d-tiled kernels for d = 384 / 512 have no causal mode)")
    D = kernel_head_dim(d)
    if q.numel() == 0:
        return o
    if not all(t.is_contiguous() for t in (q, k, v, o)):  # no strided causal kernel
        return _via_contiguous(attention_v1, q, k, v, o, causal=True)
    qp, kp, vp = (_pad_d(t, D) for t in (q, k, v))
    op = o if D == d else torch.empty((B, H, L, D), dtype=q.dtype, device=q.device)
    _launched(lib().fa_fwd_v1_causal(_ptr(qp), _ptr(kp), _ptr(vp), _ptr(op), B, H, L, D, 1.0 / d ** 0.5,
                                     _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


def _attention_v1_gqa(q, k, v, o, causal):
    """attention_v1 with H_kv < H after the common checks: fa_fwd_v1_gqa on contiguous tensors
    of a kernel head dim, zero-padded or copied to that form otherwise."""
    B, H, L, d = q.shape
    Hkv = k.shape[1]
    if q.dtype == torch.float64:
        raise NotImplementedError("grouped-query attention (GQA): float64 tensors are not supported (the fp64 "
                                  "kernels read one K/V head per query head; use bfloat16 or float16)")
    if d > 256:
        raise NotImplementedError(f"grouped-query attention (GQA): head dim d={d} is not supported (1 <= d <= "
                                  "256; the d-tiled kernels for d = 384 / 512 have no GQA form)")
    D = kernel_head_dim(d)
    if q.numel() == 0:
        return o
    # (no strided GQA kernel: views are copied, as the causal path does)
    qp, kp, vp = (_pad_d(t.contiguous(), D) for t in (q, k, v))
    op = o if D == d and o.is_contiguous() else torch.empty((B, H, L, D), dtype=q.dtype, device=q.device)
    _launched(lib().fa_fwd_v1_gqa(_ptr(qp), _ptr(kp), _ptr(vp), _ptr(op), B, H, Hkv, L, D, 1.0 / d ** 0.5,
                                  _lib.FA_FWD_CAUSAL if causal else 0, _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


@_on_tensor_device
def attention_v1(q, k, v, out=None, causal=False):
    """FA-v1 fused forward: O = softmax(q k^T / sqrt(d)) v.  Any 1 <= d <= 256 (head dims
    without a kernel are zero-padded to the next one, see kernel_head_dim).  q, k, v and out
    may be strided [B, H, L, d] views with a contiguous d -- e.g. ``x.transpose(1, 2)`` of a
    [B, L, H, d] tensor -- which the kernel addresses in place (fa_fwd_v1_ex).

    ``causal=True``: row i attends to keys 0..i only (fa_fwd_v1_causal; bfloat16 / float16,
    d <= 256 -- float64 and wider head dims raise NotImplementedError; strided views are
    copied to contiguous tensors first).

    Grouped-query attention (GQA / MQA): k and v may be ``[B, H_kv, L, d]`` with H a multiple of
    H_kv; query head h reads K/V head h // (H // H_kv), the ``repeat_interleave`` convention,
    without expanding k and v (fa_fwd_v1_gqa; bfloat16 / float16, d <= 256, causal or not;
    strided views are copied first).  H_kv == H takes the paths above."""
    if _check_qkv(q, k, v, strided=True, gqa=True) > 1:
        return _attention_v1_gqa(q, k, v, _out(out, q, strided=True), causal)
    o = _out(out, q, strided=True)
    if causal:
        return _attention_v1_causal(q, k, v, o)
    B, H, L, d = q.shape
    D = kernel_head_dim(d)
    if q.numel() == 0:  # no rows: nothing to launch (the reference returns an empty O)
        return o
    st = _stride_args(q, k, v, o) if D == d else None
    if st is not None and D in WIDE_HEAD_DIMS:
        st = False  # the d-tiled kernels address contiguous tensors only
    if st is False:
        return _via_contiguous(attention_v1, q, k, v, o)
    if D == d:
        if st is None:
            _launched(lib().fa_fwd_v1(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, L, d, _DTYPES[q.dtype], _stream(q)))
        else:
            _launched(lib().fa_fwd_v1_ex(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, L, d, st[0], st[1], st[2],
                                     1.0 / d ** 0.5, _DTYPES[q.dtype], _stream(q)))
        return o
    qp, kp, vp = (_pad_d(t, D) for t in (q, k, v))
    op = torch.empty((B, H, L, D), dtype=q.dtype, device=q.device)
    _launched(lib().fa_fwd_v1_scaled(_ptr(qp), _ptr(kp), _ptr(vp), _ptr(op), B, H, L, D, 1.0 / d ** 0.5,
                                 _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


VARLEN_MAX_TOKEN_STRIDE = 1 << 20  # elements between token rows the varlen kernel addresses in place


def _varlen_strides(ts, d):
    """{token, head} element strides of [T, H, d] tensors the varlen kernel can address in place,
    or None: d contiguous, strides positive multiples of 8 elements, token stride >= d and within
    VARLEN_MAX_TOKEN_STRIDE, 16-byte aligned base."""
    for t in ts:
        st = t.stride()
        if not (st[2] == 1 and st[0] > 0 and st[1] > 0 and st[0] % 8 == 0 and st[1] % 8 == 0 and st[0] >= d
                and st[0] <= VARLEN_MAX_TOKEN_STRIDE and t.data_ptr() % 16 == 0):
            return None
    return tuple((ctypes.c_int64 * 2)(*t.stride()[:2]) for t in ts)


@_on_tensor_device
def attention_varlen(q, k, v, cu_seqlens, max_seqlen, causal=False, out=None, *, cu_seqlens_k=None,
                     max_seqlen_k=None, seqused_k=None):
    """Variable-length (token-packed) self-attention, one launch for a ragged batch
    (fa_fwd_varlen): q ``[T, H, d]``, k and v ``[T, H_kv, d]``, bfloat16 or float16, H a multiple
    of H_kv (query head h reads K/V head h // (H // H_kv)).  ``cu_seqlens``: int32 ``[B + 1]`` on
    q's device; sequence b owns token rows ``cu_seqlens[b] : cu_seqlens[b+1]`` of q, k, v and the
    output, and attends to its own keys only -- all of them, or with ``causal=True`` those up to
    the token's own position.  Returns ``[T, H, d]``.

    cu_seqlens is never read on the host (no synchronisation); the device clamps every offset and
    length to the T rows and to ``max_seqlen``, so a corrupt array gives a wrong result, never an
    access outside the tensors.  ``max_seqlen`` is an upper bound of the lengths: it sizes the grid
    (B * H * ceil(max_seqlen / 128) workgroups, those past a sequence's end exit at once) and a
    longer sequence is truncated to it.  Rows of the output that belong to no sequence -- past
    ``cu_seqlens[-1]``, or past ``max_seqlen`` inside a sequence -- are left untouched.

    q, k, v and out are read and written in place when d is contiguous, the token and head
    strides are multiples of 8 elements (token stride at most 2**20), k and v share strides and
    the bases are 16-byte aligned -- e.g. the three slices of a fused ``[T, (H + 2 H_kv) * d]``
    QKV projection viewed as ``[T, heads, d]``; other views are copied.

    d = 32, 64, 128 and 256 run natively; any other d <= 256 is zero-padded to the next of them
    with the scale 1/sqrt(d) kept -- that COPIES q, k and v on every call: a convenience, not a
    fast path.  d > 256 and float64 raise NotImplementedError.

    Key lengths of their own -- chunked prefill against a prefix, prefix caching, verification of a
    long draft, ragged cross-attention (fa_fwd_varlen_kv).  With ``cu_seqlens_k`` (int32 ``[B + 1]``
    on q's device) and ``max_seqlen_k`` (a required int then: an upper bound of the key lengths,
    longer ranges are truncated to it), k and v are ``[Tk, H_kv, d]`` with any Tk, sequence b's keys
    are rows ``cu_seqlens_k[b] : cu_seqlens_k[b+1]`` of them, and ``cu_seqlens`` / ``max_seqlen``
    describe q and the output only.  ``seqused_k`` (int32 ``[B]`` on q's device, only together with
    ``cu_seqlens_k``) cuts sequence b's keys to the first ``seqused_k[b]`` rows of its range, clamped
    to ``[0, range]`` on the device: a padded ``[B, Lmax, H_kv, d]`` cache is read in place as
    ``cache.view(B * Lmax, H_kv, d)`` with ``cu_seqlens_k = arange(B + 1) * Lmax``.  With len_q query
    and len_k key tokens and s = len_k - len_q, every query row sees all len_k keys, or with
    ``causal=True`` position i sees keys j <= i + s -- the diagonal is aligned bottom-right, as in
    attention_decode.  A row that sees no key (len_k = 0; causal with s < 0 and i < -s) is written
    as zeros, never NaN.  Nothing is read on the host; the key side is clamped on the device like
    the query side, and k / v are addressed in place under the rules above with strides of their
    own.  With all three left None the call is the self-attention form above, unchanged."""
    # (shapes and dtypes first, so that a malformed call is named as such wherever its tensors live)
    kv_lens = cu_seqlens_k is not None
    if seqused_k is not None and not kv_lens:
        raise ValueError("seqused_k is only valid together with cu_seqlens_k")
    if max_seqlen_k is not None and not kv_lens:
        raise ValueError("max_seqlen_k is only valid together with cu_seqlens_k")
    if kv_lens and max_seqlen_k is None:
        raise ValueError("cu_seqlens_k needs max_seqlen_k (an upper bound of the key lengths)")
    for name, t in (("q", q), ("k", k), ("v", v), ("cu_seqlens", cu_seqlens), ("cu_seqlens_k", cu_seqlens_k),
                    ("seqused_k", seqused_k)):
        if not isinstance(t, torch.Tensor) and not (t is None and name in ("cu_seqlens_k", "seqused_k")):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 3:
            raise ValueError(f"{name} must be 3-D [tokens, heads, d], got shape {tuple(t.shape)}")
    if q.dtype not in _DTYPES:
        raise ValueError(f"q dtype {q.dtype} unsupported (bfloat16 or float16)")
    if k.shape != v.shape:
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} must have the same shape")
    if (q.shape[0] != k.shape[0] and not kv_lens) or q.shape[2] != k.shape[2]:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on the tokens T or d"
                         " (a k / v token count of its own needs cu_seqlens_k)")
    T, H, d = q.shape
    Hkv = k.shape[1]
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"attention_varlen: H={H} query heads are not a multiple of H_kv={Hkv} K/V heads")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
        raise ValueError(f"cu_seqlens must be an int32 tensor of shape (B + 1,), got {cu_seqlens.dtype} "
                         f"{tuple(cu_seqlens.shape)}")
    if kv_lens:
        B1 = cu_seqlens.numel()
        if cu_seqlens_k.dtype != torch.int32 or cu_seqlens_k.dim() != 1 or cu_seqlens_k.numel() != B1:
            raise ValueError(f"cu_seqlens_k must be an int32 tensor of shape (B + 1,) = ({B1},), got "
                             f"{cu_seqlens_k.dtype} {tuple(cu_seqlens_k.shape)}")
        if seqused_k is not None and (seqused_k.dtype != torch.int32 or seqused_k.dim() != 1
                                      or seqused_k.numel() != B1 - 1):
            raise ValueError(f"seqused_k must be an int32 tensor of shape (B,) = ({B1 - 1},), got {seqused_k.dtype} "
                             f"{tuple(seqused_k.shape)}")
        max_seqlen_k = int(max_seqlen_k)
        if max_seqlen_k < 0:
            raise ValueError(f"max_seqlen_k={max_seqlen_k} must not be negative")
    _check_tensor("q", q, ndim=3, strided=True)
    _check_tensor("k", k, q.dtype, q.device, ndim=3, strided=True)
    _check_tensor("v", v, q.dtype, q.device, ndim=3, strided=True)
    _check_tensor("cu_seqlens", cu_seqlens, torch.int32, q.device, ndim=1)
    if kv_lens:
        _check_tensor("cu_seqlens_k", cu_seqlens_k, torch.int32, q.device, ndim=1)
        if seqused_k is not None:
            _check_tensor("seqused_k", seqused_k, torch.int32, q.device, ndim=1)
    B = cu_seqlens.numel() - 1
    max_seqlen = int(max_seqlen)
    if max_seqlen < 0:
        raise ValueError(f"max_seqlen={max_seqlen} must not be negative")
    if q.dtype == torch.float64:
        raise NotImplementedError("attention_varlen: float64 tensors are not supported (use bfloat16 or float16)")
    if d > 256:
        raise NotImplementedError(f"attention_varlen: head dim d={d} is not supported (1 <= d <= 256)")
    o = _out(out, q, strided=True)
    if q.numel() == 0 or B == 0 or max_seqlen == 0:  # no rows, no sequences: nothing to launch
        return o
    D = kernel_head_dim(d)
    if D != d:
        q, k, v = (_pad_d(t, D) for t in (q, k, v))
    Tk = k.shape[0]
    if kv_lens and (Tk == 0 or max_seqlen_k == 0):
        # no key anywhere: every row of a sequence is zeros (the kernel's rule, total_tokens_k = 0);
        # k and v are never read, one row stands in for their null pointers
        k = v = torch.empty((1, Hkv, D), dtype=q.dtype, device=q.device)
        Tk, max_seqlen_k = 0, 1
    st = _varlen_strides((q, k, o), D) if D == d and k.stride() == v.stride() else None
    if st is None:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if D != d or _varlen_strides((o,), D) is None:
            # rows of no sequence keep what out holds: the kernel's output starts as a copy of it
            op = torch.empty((T, H, D), dtype=q.dtype, device=q.device)
            if out is not None:
                op[..., :d].copy_(o)
        else:
            op = o
        st = _varlen_strides((q, k, op), D)
    else:
        op = o
    if kv_lens:
        _launched(lib().fa_fwd_varlen_kv(_ptr(q), _ptr(k), _ptr(v), _ptr(op), _ptr(cu_seqlens), _ptr(cu_seqlens_k),
                                         None if seqused_k is None else _ptr(seqused_k), B, T, Tk, max_seqlen,
                                         max_seqlen_k, H, Hkv, D, st[0], st[1], st[2], 1.0 / d ** 0.5,
                                         _lib.FA_FWD_CAUSAL if causal else 0, _DTYPES[q.dtype], _stream(q)))
        return _unpad_into(op, o, d)
    _launched(lib().fa_fwd_varlen(_ptr(q), _ptr(k), _ptr(v), _ptr(op), _ptr(cu_seqlens), B, T, max_seqlen, H, Hkv, D,
                                  st[0], st[1], st[2], 1.0 / d ** 0.5, _lib.FA_FWD_CAUSAL if causal else 0,
                                  _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


def _d_tiles(d, d_tile_qk, d_tile_v):
    """d tiles the caller left as None: min(32, d) up to d = 256 (the reference's D_TILE = 32
    where d allows it; there the tiles are only validated -- one LDS tile holds a whole row),
    128 above, where the d-tiled kernel streams K / V in tile-wide column chunks.  The output
    is bitwise the same for every tile choice, only the speed differs: d = 512 B32 H8 L1024,
    32/32 0.931 ms against 128/128 0.682 ms (24 chunk waits + barriers per 64-key tile against
    6; scripts/dtile_sweep.py, profiles/r05/dtile_sweep.txt)."""
    dflt = min(32, d) if d <= 256 else 128
    return (dflt if d_tile_qk is None else int(d_tile_qk),
            dflt if d_tile_v is None else int(d_tile_v))


@_on_tensor_device
def attention_tiled_d(q, k, v, d_tile_qk=None, d_tile_v=None, out=None):
    """FA-v1 d-tiled forward (O_acc in VGPRs); d tiles as in the reference launcher
    (0 < d_tile <= d; default min(32, d) up to d = 256, 128 above -- see _d_tiles).  d <= 256: one LDS tile holds a whole row and the
    fused kernel runs (tiles validated); 256 < d <= 512: the d-tiled kernel streams K and V
    through LDS in d_tile-wide column chunks (rounded down to 32, 64 or 128 columns)."""
    _check_qkv(q, k, v, strided=True)
    B, H, L, d = q.shape
    d_tile_qk, d_tile_v = _d_tiles(d, d_tile_qk, d_tile_v)
    # the tile arguments are validated against the true d, as the launcher does
    # (flash_attention_v1_tiled_d/CUDA/flash_attention_v1.h:326-327)
    for name, t in (("d_tile_qk", d_tile_qk), ("d_tile_v", d_tile_v)):
        if not 0 < int(t) <= d:
            raise _lib.FaArgumentError(1, f"{name}={int(t)} must satisfy 0 < {name} <= d={d}")
    D = kernel_head_dim(d)
    if D not in WIDE_HEAD_DIMS:
        if q.numel() == 0 or D != d or not all(t.is_contiguous() for t in (q, k, v)) or (
                out is not None and not out.is_contiguous()):
            # padded head dims and strided views run on fa_fwd_v1's paths (the same kernel)
            return attention_v1(q, k, v, out=out)
        o = _out(out, q)
        _launched(lib().fa_fwd_v1_tiled_d(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, L, d, int(d_tile_qk),
                                      int(d_tile_v), _DTYPES[q.dtype], _stream(q)))
        return o
    o = _out(out, q, strided=True)
    if q.numel() == 0:
        return o
    qc, kc, vc = (_pad_d(t.contiguous(), D) for t in (q, k, v))
    oc = o if D == d and o.is_contiguous() else torch.empty((B, H, L, D), dtype=q.dtype, device=q.device)
    _launched(lib().fa_fwd_v1_tiled_d_scaled(_ptr(qc), _ptr(kc), _ptr(vc), _ptr(oc), B, H, L, D, int(d_tile_qk),
                                         int(d_tile_v), 1.0 / d ** 0.5, _DTYPES[q.dtype], _stream(q)))
    if oc is not o:
        o.copy_(oc[..., :d])
    return o


def _kvtpb(kv_tiles_per_block):
    return FA_KV_TILES_AUTO if kv_tiles_per_block == "auto" else int(kv_tiles_per_block)


def _bpw(blocks_per_workgroup):
    g = FA_BLOCKS_PER_WG_AUTO if blocks_per_workgroup is None else int(blocks_per_workgroup)
    if g < 0:
        raise ValueError(f"blocks_per_workgroup={g} must be >= 1 (or None for the library's grouping)")
    return g


def v2_workspace_bytes(B, H, L, d, kv_tiles_per_block=4, dtype=torch.bfloat16,
                       partial_dtype=None, blocks_per_workgroup=None):
    """(bytes, num_splits) of the split-KV workspace: num_splits = the reference's key blocks;
    the bytes cover the partials actually combined through the workspace (v2_split_plan) in
    partial_dtype (per-row scaled fp16 by default; fp64 for fp64 inputs)."""
    pd = _default_pdtype(dtype, partial_dtype, fused=True)
    kv_tiles_per_block = _kvtpb(kv_tiles_per_block)
    nbytes = ctypes.c_size_t()
    ns = ctypes.c_int()
    d = kernel_head_dim(d)
    check(lib().fa_fwd_v2_workspace_size_ex(B, H, L, d, int(kv_tiles_per_block), _bpw(blocks_per_workgroup),
                                            _DTYPES[dtype], _PDTYPES[pd], ctypes.byref(nbytes), ctypes.byref(ns)))
    return nbytes.value, ns.value


def v2_split_plan(B, H, L, d, kv_tiles_per_block=4, dtype=torch.bfloat16, blocks_per_workgroup=None):
    """(key_blocks, blocks_per_workgroup, partials_per_tile) of fa_fwd_v2's schedule: the
    reference's key blocks of kv_tiles_per_block tiles, how many consecutive blocks one
    workgroup combines on chip, and how many partial workgroups per query tile are combined
    through the workspace.  ``blocks_per_workgroup`` None: the library's grouping; n >= 1 fixes
    it (1 = one workgroup and one HBM partial per key block, the reference's layout)."""
    kb, g, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().fa_fwd_v2_split_plan(B, H, L, kernel_head_dim(d), int(_kvtpb(kv_tiles_per_block)),
                                     _bpw(blocks_per_workgroup), _DTYPES[dtype],
                                     ctypes.byref(kb), ctypes.byref(g), ctypes.byref(p)))
    return kb.value, g.value, p.value


@_on_tensor_device
def attention_v2(q, k, v, kv_tiles_per_block=4, d_tile_qk=None, d_tile_v=None, partial_dtype=None,
                 out=None, workspace=None, blocks_per_workgroup=None, workspace_zeroed=False):
    """FA-v2 split-KV forward (partial kernel + combine kernel).

    A split is ``kv_tiles_per_block`` KV tiles of the kernel's own tile size (64 keys;
    32 at d = 256); ``kv_tiles_per_block="auto"`` lets the library pick the split from the
    device's occupancy (no split when the query tiles already fill the GPU).
    ``blocks_per_workgroup`` (None: the library's grouping, v2_split_plan) fixes how many
    consecutive key blocks one workgroup combines on chip; 1 is the reference's layout (one
    HBM partial per key block).
    Partial outputs are kept as per-row scaled fp16 by default (``PARTIAL_FP16_SCALED``: half
    the workspace traffic of ``torch.float32``, 11 significant bits relative to each row's
    largest partial, no fp16 range limit); ``torch.float32`` or the input dtype on request.
    ``workspace`` (a uint8 device tensor) is allocated from torch's caching allocator when
    not given, so the call itself never reaches hipMalloc after warm-up.
    ``workspace_zeroed=True`` promises that the workspace came zeroed (``torch.zeros``) and has
    been used since only by attention_v2 calls of this same shape and plan (each leaves its
    counters zero): the per-call counter reset, a dispatch of its own, is skipped
    (fa_fwd_v2_ex2 with FA_V2_COUNTERS_ZERO; 1.6-1.8 us per call).
    """
    _check_qkv(q, k, v, strided=True)
    o = _out(out, q, strided=True)
    B, H, L, d = q.shape
    D = kernel_head_dim(d)
    d_tile_qk, d_tile_v = _d_tiles(d, d_tile_qk, d_tile_v)
    if q.numel() == 0:  # no rows: nothing to launch
        return o
    st = _stride_args(q, k, v, o) if D == d else None
    if st is not None and D in WIDE_HEAD_DIMS:
        st = False  # the d-tiled kernels address contiguous tensors only
    if st is False:
        return _via_contiguous(attention_v2, q, k, v, o, kv_tiles_per_block=kv_tiles_per_block,
                               d_tile_qk=d_tile_qk, d_tile_v=d_tile_v, partial_dtype=partial_dtype,
                               workspace=workspace, blocks_per_workgroup=blocks_per_workgroup,
                               workspace_zeroed=workspace_zeroed)
    pd = _default_pdtype(q.dtype, partial_dtype, fused=True)
    kv_tiles_per_block = _kvtpb(kv_tiles_per_block)
    bpw = _bpw(blocks_per_workgroup)
    nbytes, _ = v2_workspace_bytes(B, H, L, d, kv_tiles_per_block, q.dtype, pd, bpw)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        workspace_zeroed = False
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"workspace too small: {nbytes} bytes needed")
    wsb = workspace.numel() * workspace.element_size()
    flags = _lib.FA_V2_COUNTERS_ZERO if workspace_zeroed else 0
    if D == d:
        sq, skv, so = (None, None, None) if st is None else st
        _launched(lib().fa_fwd_v2_ex2(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, H, L, d, int(d_tile_qk),
                                      int(d_tile_v), int(kv_tiles_per_block), bpw, _ptr(workspace), wsb, sq, skv,
                                      so, 1.0 / d ** 0.5, _DTYPES[q.dtype], _PDTYPES[pd], flags, _stream(q)))
        return o
    for name, t in (("d_tile_qk", d_tile_qk), ("d_tile_v", d_tile_v)):
        if not 0 < int(t) <= d:
            raise _lib.FaArgumentError(1, f"{name}={int(t)} must satisfy 0 < {name} <= d={d}")
    qp, kp, vp = (_pad_d(t, D) for t in (q, k, v))
    op = torch.empty((B, H, L, D), dtype=q.dtype, device=q.device)
    _launched(lib().fa_fwd_v2_ex2(_ptr(qp), _ptr(kp), _ptr(vp), _ptr(op), B, H, L, D, int(d_tile_qk),
                                  int(d_tile_v), int(kv_tiles_per_block), bpw, _ptr(workspace), wsb, None, None, None,
                                  1.0 / d ** 0.5, _DTYPES[q.dtype], _PDTYPES[pd], flags, _stream(q)))
    return _unpad_into(op, o, d)


@_on_tensor_device
def attention_partial(q, k, v, chunk_rows=None, partial_dtype=None, o_part=None, lse=None):
    """Split-KV partial over one whole key range (k, v: [B, H, Lk, d]).

    Returns ``(o_part, lse)`` with o_part ``[Lq/chunk_rows, B*H, chunk_rows, d]`` holding the
    normalised partial output and lse ``[Lq/chunk_rows, B*H, chunk_rows]`` its base-2
    log-sum-exp (of the scores times log2(e)/sqrt(d)); fp32 partials and lse by default,
    fp64 for fp64 inputs.  ``partial_dtype=PARTIAL_FP16_SCALED``: o_part is fp16 holding each
    row times 2^-e (the row's largest |value| just below 1) and lse gains a trailing dim of 2,
    ``{lse, e}`` per row -- ``combine`` recognises the format by that dim.
    """
    _check_qkv(q, k, v, same_len=False, strided=True)
    if not (k.is_contiguous() and v.is_contiguous()):
        k, v = k.contiguous(), v.contiguous()
    qst = None
    if not q.is_contiguous():  # a row range of a longer q (the multi-GPU chunks): in place
        st = _stride_args(q, k, v, q)
        if st is False:
            q = q.contiguous()
        else:
            qst = st[0]
    B, H, Lq, d = q.shape
    Lk = k.shape[2]
    cr = Lq if chunk_rows is None else int(chunk_rows)
    if cr <= 0 or Lq % cr:
        raise ValueError(f"chunk_rows={cr} must divide Lq={Lq}")
    nch = Lq // cr
    partial_dtype = _default_pdtype(q.dtype, partial_dtype)
    lse_dtype = torch.float64 if q.dtype == torch.float64 else torch.float32
    scaled = partial_dtype == PARTIAL_FP16_SCALED
    o_part = _out(o_part, q, (nch, B * H, cr, d), torch.float16 if scaled else partial_dtype)
    lse = _out(lse, q, (nch, B * H, cr, 2) if scaled else (nch, B * H, cr), lse_dtype)
    if qst is None:
        _launched(lib().fa_fwd_partial(_ptr(q), _ptr(k), _ptr(v), _ptr(o_part), _ptr(lse), B, H, Lq, Lk, d,
                                   cr, _DTYPES[q.dtype], _PDTYPES[partial_dtype], _stream(q)))
    else:
        _launched(lib().fa_fwd_partial_ex(_ptr(q), _ptr(k), _ptr(v), _ptr(o_part), _ptr(lse), B, H, Lq, Lk, d,
                                      cr, qst, _DTYPES[q.dtype], _PDTYPES[partial_dtype], _stream(q)))
    return o_part, lse


@_on_tensor_device
def combine(o_part, lse, B, H, dtype, out=None):
    """Combine ``S`` partials o_part ``[S, B*H, L, d]`` / lse ``[S, B*H, L]`` -> ``[B, H, L, d]``.

    An lse of shape ``[S, B*H, L, 2]`` marks fp16 per-row scaled partials (``attention_partial``
    with ``PARTIAL_FP16_SCALED``)."""
    _check_tensor("o_part", o_part, ndim=4)
    scaled = lse.dim() == 4
    _check_tensor("lse", lse, torch.float64 if o_part.dtype == torch.float64 else torch.float32,
                  o_part.device, ndim=4 if scaled else 3)
    S, BH, L, d = o_part.shape
    if BH != B * H or tuple(lse.shape) != ((S, BH, L, 2) if scaled else (S, BH, L)):
        raise ValueError(f"inconsistent shapes o_part {tuple(o_part.shape)} lse {tuple(lse.shape)} "
                         f"B={B} H={H}")
    if scaled and o_part.dtype != torch.float16:
        raise ValueError(f"scaled partials (lse [..., 2]) are fp16, got {o_part.dtype}")
    o = _out(out, o_part, (B, H, L, d), dtype)
    pd = PARTIAL_FP16_SCALED if scaled else o_part.dtype
    _launched(lib().fa_combine(_ptr(o_part), _ptr(lse), _ptr(o), S, B, H, L, d, _DTYPES[dtype],
                           _PDTYPES[pd], _stream(o_part)))
    return o


DECODE_HEAD_DIMS = (64, 128)  # head dims with a decode kernel
DECODE_MAX_ROWS = 64          # packed query rows (H / H_kv) * Lq of one K/V head at most


def decode_plan(B, H, H_kv, Lq, Lk, d, num_splits=None, dtype=torch.bfloat16, cus=None):
    """``(splits, keys_per_split, workspace_bytes)`` attention_decode uses for this problem
    (fa_fwd_decode_plan): ``num_splits=None`` lets the library pick as few key splits as still
    give every compute unit a workgroup (1 when B * H_kv alone does).  ``cus``: the compute
    units to plan for, None = the current device's (needs no device when given).  d is the
    kernel's head dim (64 or 128)."""
    splits, kps, nbytes = _lib._I(), _lib._I(), ctypes.c_size_t()
    check(lib().fa_fwd_decode_plan(int(B), int(H), int(H_kv), int(Lq), int(Lk), int(d),
                                   0 if num_splits is None else int(num_splits), 0 if cus is None else int(cus),
                                   _DTYPES[dtype], ctypes.byref(splits), ctypes.byref(kps), ctypes.byref(nbytes)))
    return splits.value, kps.value, nbytes.value


@_on_tensor_device
def attention_decode(q, k, v, seqlens_k=None, causal=True, num_splits=None, out=None, workspace=None):
    """KV-cache decode attention: q ``[B, H, Lq, d]`` (Lq small) against k, v ``[B, H_kv, Lk, d]``,
    bfloat16 or float16, H a multiple of H_kv (query head h reads K/V head h // (H // H_kv)) and
    (H // H_kv) * Lq <= 64 -- the query rows of a K/V head are packed into one tile, the keys are
    split over the chip and combined in the same call (fa_fwd_decode).

    ``seqlens_k``: int32 ``[B]`` tensor on q's device, the valid keys of each sequence (clamped
    to [0, Lk] on the device; no host read); rows of k / v from there on are never used, whatever
    they hold.  ``causal`` (default): the mask aligned bottom-right, row position i sees keys
    j <= len_b - Lq + i -- a no-op at Lq = 1; a row without a visible key is zero.
    ``num_splits``: key splits (None: from the device's occupancy, see decode_plan).

    k and v are read in place through their strides when d is contiguous, k and v share strides
    that are multiples of 8 elements and the base is 16-byte aligned -- e.g. a ``[B, Lmax, H_kv,
    d]`` cache as ``cache.transpose(1, 2)[:, :, :Lk]``; other views are copied.  q and out are
    small and copied when not contiguous.  ``workspace``: a uint8 device tensor of at least
    decode_plan(...)[2] bytes; with it (and ``out``) the call allocates nothing.

    d = 64 and 128 run natively; any other d <= 128 is zero-padded to the next of them with the
    scale 1/sqrt(d) kept -- that COPIES the cache on every call: a convenience, not a fast path.
    d > 128, float64 and (H // H_kv) * Lq > 64 raise NotImplementedError."""
    _check_tensor("q", q, strided=True)
    if q.dtype not in _DTYPES:
        raise ValueError(f"q dtype {q.dtype} unsupported (bfloat16 or float16)")
    _check_tensor("k", k, q.dtype, q.device, strided=True)
    _check_tensor("v", v, q.dtype, q.device, strided=True)
    if k.shape != v.shape:
        raise ValueError(f"k {tuple(k.shape)} and v {tuple(v.shape)} must have the same shape")
    if q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError(f"q {tuple(q.shape)} and k {tuple(k.shape)} disagree on B or d")
    B, H, Lq, d = q.shape
    Hkv, Lk = k.shape[1], k.shape[2]
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"attention_decode: H={H} query heads are not a multiple of H_kv={Hkv} K/V heads")
    if q.dtype == torch.float64:
        raise NotImplementedError("attention_decode: float64 tensors are not supported (use bfloat16 or float16)")
    if d > DECODE_HEAD_DIMS[-1]:
        raise NotImplementedError(f"attention_decode: head dim d={d} is not supported (1 <= d <= 128)")
    if (H // Hkv) * Lq > DECODE_MAX_ROWS:
        raise NotImplementedError(f"attention_decode: (H / H_kv) * Lq = {H // Hkv} * {Lq} packed query rows exceed "
                                  f"{DECODE_MAX_ROWS}; long queries are served by attention_v1")
    if seqlens_k is not None:
        _check_tensor("seqlens_k", seqlens_k, torch.int32, q.device, ndim=1)
        if seqlens_k.dtype != torch.int32 or tuple(seqlens_k.shape) != (B,):
            raise ValueError(f"seqlens_k must be an int32 tensor of shape ({B},), got {seqlens_k.dtype} "
                             f"{tuple(seqlens_k.shape)}")
    o = _out(out, q, strided=True)
    if q.numel() == 0:
        return o
    if Lk == 0:  # no keys: every row is empty
        return o.zero_()
    D = next(x for x in DECODE_HEAD_DIMS if x >= d)
    kst = None
    if D != d:
        k, v = _pad_d(k, D), _pad_d(v, D)
    elif not (k.is_contiguous() and v.is_contiguous()):
        st = k.stride()
        if (k.stride() == v.stride() and st[3] == 1 and all(x > 0 and x % 8 == 0 for x in st[:3]) and st[2] >= d
                and st[2] <= 1 << 20 and k.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0):
            kst = (ctypes.c_int64 * 3)(*st[:3])
        else:
            k, v = k.contiguous(), v.contiguous()
    qp = _pad_d(q.contiguous(), D)
    op = o if D == d and o.is_contiguous() else torch.empty((B, H, Lq, D), dtype=q.dtype, device=q.device)
    ns = 0 if num_splits is None else int(num_splits)
    if ns < 0:
        raise ValueError(f"num_splits={ns} must be positive (or None)")
    nbytes = decode_plan(B, H, Hkv, Lq, Lk, D, ns, q.dtype)[2]
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    else:
        _check_tensor("workspace", workspace, torch.uint8, q.device, ndim=1)
        if workspace.numel() * workspace.element_size() < nbytes:
            raise ValueError(f"workspace too small: {nbytes} bytes needed")
    _launched(lib().fa_fwd_decode(_ptr(qp), _ptr(k), _ptr(v), _ptr(op), None if seqlens_k is None else _ptr(seqlens_k),
                                  B, H, Hkv, Lq, Lk, D, kst, 1.0 / d ** 0.5, _lib.FA_FWD_CAUSAL if causal else 0, ns,
                                  None if workspace is None else _ptr(workspace),
                                  0 if workspace is None else workspace.numel() * workspace.element_size(),
                                  _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


DECODE_PAGE_MULTIPLE = 64     # keys per page: a multiple of the decode kernel's key tile


@_on_tensor_device
def attention_decode_paged(q, k_cache, v_cache, block_table, seqlens_k=None, max_seqlen_k=None, causal=True,
                           num_splits=None, out=None, workspace=None):
    """attention_decode on a paged KV cache, read in place through a block table
    (fa_fwd_decode_paged): q ``[B, H, Lq, d]`` against pools k_cache, v_cache ``[num_blocks,
    page_size, H_kv, d]``, bfloat16 or float16.  Key j of sequence b is row ``j % page_size`` of
    block ``block_table[b, j // page_size]``; the result is exactly (bit for bit) attention_decode
    on the cache gathered in table order, with the same ``seqlens_k``, ``causal``, ``num_splits``,
    ``out`` and ``workspace`` (decode_plan with Lk = max_seqlen_k).

    ``block_table``: int32 ``[B, P]`` on q's device, last dim contiguous, any row stride.  Only the
    entries of pages that hold a key below len_b are read (the rest may be -1 or anything), and
    every entry read is clamped to [0, num_blocks - 1] on the device: a corrupt table gives a
    wrong result, never an access outside the pool.  ``max_seqlen_k`` (None: P * page_size): the
    upper bound the lengths are clamped to and the split plan is made for; at most P * page_size.

    The pool is never copied: any strides are taken when d is contiguous, k_cache and v_cache
    share strides that are multiples of 8 elements and the bases are 16-byte aligned -- a
    ``[num_blocks, H_kv, page_size, d]`` pool goes in as ``pool.transpose(1, 2)``.  Other views,
    page_size not a multiple of 64, d other than 64 / 128 (no padding copy of a whole pool),
    float64 and (H // H_kv) * Lq > 64 raise NotImplementedError.  q and out are small and copied
    when not contiguous; with ``out`` and ``workspace`` given the call allocates nothing."""
    _check_tensor("q", q, strided=True)
    if q.dtype not in _DTYPES:
        raise ValueError(f"q dtype {q.dtype} unsupported (bfloat16 or float16)")
    _check_tensor("k_cache", k_cache, q.dtype, q.device, strided=True)
    _check_tensor("v_cache", v_cache, q.dtype, q.device, strided=True)
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} must have the same shape")
    if q.shape[3] != k_cache.shape[3]:
        raise ValueError(f"q {tuple(q.shape)} and k_cache {tuple(k_cache.shape)} disagree on d")
    B, H, Lq, d = q.shape
    nblk, ps, Hkv = k_cache.shape[:3]
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"attention_decode_paged: H={H} query heads are not a multiple of H_kv={Hkv} K/V heads")
    if q.dtype == torch.float64:
        raise NotImplementedError("attention_decode_paged: float64 tensors are not supported (use bfloat16 or float16)")
    if d not in DECODE_HEAD_DIMS:
        raise NotImplementedError(f"attention_decode_paged: head dim d={d} is not supported (64 or 128; a pool is "
                                  "not padded)")
    if ps <= 0 or ps % DECODE_PAGE_MULTIPLE:
        raise NotImplementedError(f"attention_decode_paged: page_size={ps} is not a multiple of {DECODE_PAGE_MULTIPLE} "
                                  "keys (pages of 16 / 32 keys have no kernel)")
    if (H // Hkv) * Lq > DECODE_MAX_ROWS:
        raise NotImplementedError(f"attention_decode_paged: (H / H_kv) * Lq = {H // Hkv} * {Lq} packed query rows exceed "
                                  f"{DECODE_MAX_ROWS}; long queries are served by attention_v1")
    _check_tensor("block_table", block_table, torch.int32, q.device, ndim=2, strided=True)
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
        raise ValueError(f"block_table must be an int32 tensor of shape ({B}, pages), got {block_table.dtype} "
                         f"{tuple(block_table.shape)}")
    P = block_table.shape[1]
    if (P > 1 and block_table.stride(1) != 1) or (B > 1 and block_table.stride(0) < P):
        raise ValueError(f"block_table rows must be contiguous and at least {P} entries apart (strides "
                         f"{tuple(block_table.stride())})")
    Lk = P * ps if max_seqlen_k is None else int(max_seqlen_k)
    if Lk < 0:
        raise ValueError(f"max_seqlen_k={Lk} must not be negative")
    if Lk > P * ps:
        raise ValueError(f"max_seqlen_k={Lk} exceeds what the block table maps ({P} pages of {ps} keys)")
    if seqlens_k is not None:
        _check_tensor("seqlens_k", seqlens_k, torch.int32, q.device, ndim=1)
        if seqlens_k.dtype != torch.int32 or tuple(seqlens_k.shape) != (B,):
            raise ValueError(f"seqlens_k must be an int32 tensor of shape ({B},), got {seqlens_k.dtype} "
                             f"{tuple(seqlens_k.shape)}")
    st = k_cache.stride()
    if nblk > 0 and not (st == v_cache.stride() and st[3] == 1 and all(x > 0 and x % 8 == 0 for x in st[:3])
                         and st[1] >= d and st[1] <= 1 << 20 and k_cache.data_ptr() % 16 == 0
                         and v_cache.data_ptr() % 16 == 0):
        raise NotImplementedError(f"attention_decode_paged: the pool is read in place and this view cannot be "
                                  f"addressed (k_cache strides {tuple(st)}, v_cache strides {tuple(v_cache.stride())}): "
                                  "d contiguous, shared strides that are multiples of 8 elements, 16-byte aligned bases")
    ns = 0 if num_splits is None else int(num_splits)
    if ns < 0:
        raise ValueError(f"num_splits={ns} must be positive (or None)")
    o = _out(out, q, strided=True)
    if q.numel() == 0:
        return o
    if Lk == 0:  # no keys: every row is empty
        return o.zero_()
    if nblk == 0:
        raise ValueError("attention_decode_paged: the pool has no blocks")
    qp = q.contiguous()
    op = o if o.is_contiguous() else torch.empty((B, H, Lq, d), dtype=q.dtype, device=q.device)
    nbytes = decode_plan(B, H, Hkv, Lq, Lk, d, ns, q.dtype)[2]
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    else:
        _check_tensor("workspace", workspace, torch.uint8, q.device, ndim=1)
        if workspace.numel() * workspace.element_size() < nbytes:
            raise ValueError(f"workspace too small: {nbytes} bytes needed")
    # {block, head, row} of the [num_blocks, page_size, H_kv, d] view
    cst = (ctypes.c_int64 * 3)(st[0], st[2], st[1])
    _launched(lib().fa_fwd_decode_paged(_ptr(qp), _ptr(k_cache), _ptr(v_cache), _ptr(op), _ptr(block_table),
                                        None if seqlens_k is None else _ptr(seqlens_k), B, H, Hkv, Lq, Lk, d, nblk, ps,
                                        block_table.stride(0) if B > 1 else max(P, block_table.stride(0)), cst,
                                        1.0 / d ** 0.5, _lib.FA_FWD_CAUSAL if causal else 0, ns,
                                        None if workspace is None else _ptr(workspace),
                                        0 if workspace is None else workspace.numel() * workspace.element_size(),
                                        _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


VARLEN_PAGED_HEAD_DIMS = (32, 64, 128, 256)  # head dims of the paged varlen forward (a pool is not padded)


def _paged_pool_args(who, k_cache, v_cache, dtype, device, block_table, seqused_k, B):
    """The pool / table / key-count checks attention_varlen_paged and kv_cache_append_paged share.
    Returns (num_blocks, page_size, H_kv, P, table_stride, cache_strides {block, head, row})."""
    _check_tensor("k_cache", k_cache, dtype, device, strided=True)
    _check_tensor("v_cache", v_cache, dtype, device, strided=True)
    if k_cache.shape != v_cache.shape:
        raise ValueError(f"k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} must have the same shape")
    nblk, ps, Hkv, d = k_cache.shape
    if ps <= 0 or ps % DECODE_PAGE_MULTIPLE:
        raise NotImplementedError(f"{who}: page_size={ps} is not a multiple of {DECODE_PAGE_MULTIPLE} keys (pages of "
                                  "16 / 32 keys have no kernel)")
    _check_tensor("block_table", block_table, torch.int32, device, ndim=2, strided=True)
    if block_table.shape[0] != B:
        raise ValueError(f"block_table must be an int32 tensor of shape ({B}, pages), got {block_table.dtype} "
                         f"{tuple(block_table.shape)}")
    P = block_table.shape[1]
    if (P > 1 and block_table.stride(1) != 1) or (B > 1 and block_table.stride(0) < P):
        raise ValueError(f"block_table rows must be contiguous and at least {P} entries apart (strides "
                         f"{tuple(block_table.stride())})")
    _check_tensor("seqused_k", seqused_k, torch.int32, device, ndim=1)
    if tuple(seqused_k.shape) != (B,):
        raise ValueError(f"seqused_k must be an int32 tensor of shape ({B},), got {seqused_k.dtype} "
                         f"{tuple(seqused_k.shape)}")
    st = k_cache.stride()
    if nblk > 0 and not (st == v_cache.stride() and st[3] == 1 and all(x > 0 and x % 8 == 0 for x in st[:3])
                         and st[1] >= d and st[1] <= 1 << 20 and k_cache.data_ptr() % 16 == 0
                         and v_cache.data_ptr() % 16 == 0):
        raise NotImplementedError(f"{who}: the pool is addressed in place and this view cannot be (k_cache strides "
                                  f"{tuple(st)}, v_cache strides {tuple(v_cache.stride())}): d contiguous, shared "
                                  "strides that are multiples of 8 elements, 16-byte aligned bases")
    tstride = block_table.stride(0) if B > 1 else max(P, block_table.stride(0))
    return nblk, ps, Hkv, P, tstride, (ctypes.c_int64 * 3)(st[0], st[2], st[1])


def _check_cu_seqlens(cu_seqlens, device):
    if not isinstance(cu_seqlens, torch.Tensor):
        raise TypeError(f"cu_seqlens must be a torch.Tensor, got {type(cu_seqlens).__name__}")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
        raise ValueError(f"cu_seqlens must be an int32 tensor of shape (B + 1,), got {cu_seqlens.dtype} "
                         f"{tuple(cu_seqlens.shape)}")
    _check_tensor("cu_seqlens", cu_seqlens, torch.int32, device, ndim=1)
    return cu_seqlens.numel() - 1


@_on_tensor_device
def attention_varlen_paged(q, k_cache, v_cache, cu_seqlens, max_seqlen, block_table, seqused_k, max_seqlen_k=None,
                           causal=False, out=None):
    """attention_varlen with the keys in a paged KV cache, read in place through a block table
    (fa_fwd_varlen_paged): chunked and prefix-cached prefill against the pool attention_decode_paged
    reads, one launch, nothing read on the host.  q ``[T, H, d]`` with ``cu_seqlens`` /
    ``max_seqlen`` as in attention_varlen; pools k_cache, v_cache ``[num_blocks, page_size, H_kv,
    d]``, bfloat16 or float16.  Sequence b has ``clamp(seqused_k[b], 0, max_seqlen_k)`` keys, key j
    being row ``j % page_size`` of block ``block_table[b, j // page_size]``; with ``causal=True``
    query position i sees keys j <= i + len_k - len_q (bottom-right aligned), and a row that sees
    no key is written as zeros.  The result is exactly (bit for bit) ``attention_varlen(q, Kg, Vg,
    cu_seqlens, max_seqlen, causal, cu_seqlens_k=arange(B + 1) * Lg, max_seqlen_k=max_seqlen_k,
    seqused_k=seqused_k)`` on the cache gathered in table order into ``[B * Lg, H_kv, d]``.

    ``block_table``: int32 ``[B, P]`` on q's device, last dim contiguous, any row stride >= P.  Only
    the entries of pages that hold a key the call reads are loaded (the rest may be -1 or anything)
    and every entry is clamped to [0, num_blocks - 1] on the device: a corrupt table gives a wrong
    result, never an access outside the pool.  ``seqused_k``: int32 ``[B]``.  ``max_seqlen_k`` (None:
    P * page_size): the upper bound of the key counts, at most P * page_size.

    The pool is never copied and never padded: any strides are taken when d is contiguous, k_cache
    and v_cache share strides that are multiples of 8 elements and the bases are 16-byte aligned --
    a ``[num_blocks, H_kv, page_size, d]`` pool goes in as ``pool.transpose(1, 2)``.  Other views,
    page_size not a multiple of 64, d other than 32 / 64 / 128 / 256 and float64 raise
    NotImplementedError.  q and out follow attention_varlen's in-place / copy rules; rows of the
    output that belong to no sequence keep what ``out`` holds."""
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache), ("cu_seqlens", cu_seqlens),
                    ("block_table", block_table), ("seqused_k", seqused_k)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if q.dim() != 3:
        raise ValueError(f"q must be 3-D [tokens, heads, d], got shape {tuple(q.shape)}")
    if k_cache.dim() != 4:
        raise ValueError(f"k_cache must be 4-D [num_blocks, page_size, H_kv, d], got shape {tuple(k_cache.shape)}")
    if q.dtype not in _DTYPES:
        raise ValueError(f"q dtype {q.dtype} unsupported (bfloat16 or float16)")
    if q.shape[2] != k_cache.shape[3]:
        raise ValueError(f"q {tuple(q.shape)} and k_cache {tuple(k_cache.shape)} disagree on d")
    T, H, d = q.shape
    if block_table.dtype != torch.int32 or block_table.dim() != 2:
        raise ValueError(f"block_table must be an int32 tensor of shape (B, pages), got {block_table.dtype} "
                         f"{tuple(block_table.shape)}")
    if seqused_k.dtype != torch.int32 or seqused_k.dim() != 1:
        raise ValueError(f"seqused_k must be an int32 tensor of shape (B,), got {seqused_k.dtype} "
                         f"{tuple(seqused_k.shape)}")
    _check_tensor("q", q, ndim=3, strided=True)
    B = _check_cu_seqlens(cu_seqlens, q.device)
    if q.dtype == torch.float64:
        raise NotImplementedError("attention_varlen_paged: float64 tensors are not supported (use bfloat16 or float16)")
    if d not in VARLEN_PAGED_HEAD_DIMS:
        raise NotImplementedError(f"attention_varlen_paged: head dim d={d} is not supported (32, 64, 128 or 256; a "
                                  "pool is not padded)")
    nblk, ps, Hkv, P, tstride, cst = _paged_pool_args("attention_varlen_paged", k_cache, v_cache, q.dtype, q.device,
                                                      block_table, seqused_k, B)
    if Hkv <= 0 or H % Hkv:
        raise ValueError(f"attention_varlen_paged: H={H} query heads are not a multiple of H_kv={Hkv} K/V heads")
    max_seqlen = int(max_seqlen)
    if max_seqlen < 0:
        raise ValueError(f"max_seqlen={max_seqlen} must not be negative")
    Lk = P * ps if max_seqlen_k is None else int(max_seqlen_k)
    if Lk < 0:
        raise ValueError(f"max_seqlen_k={Lk} must not be negative")
    if Lk > P * ps:
        raise ValueError(f"max_seqlen_k={Lk} exceeds what the block table maps ({P} pages of {ps} keys)")
    o = _out(out, q, strided=True)
    if q.numel() == 0 or B == 0 or max_seqlen == 0:  # no rows, no sequences: nothing to launch
        return o
    if Lk == 0:
        # no key anywhere: every row of a sequence is zeros (the kernel's rule).  One block of zeros
        # and a zero key count stand in for the pool, which is never read
        k_cache = v_cache = torch.zeros((1, ps, Hkv, d), dtype=q.dtype, device=q.device)
        block_table = torch.zeros((B, 1), dtype=torch.int32, device=q.device)
        seqused_k = torch.zeros((B,), dtype=torch.int32, device=q.device)
        st = k_cache.stride()
        nblk, tstride, Lk, cst = 1, 1, 1, (ctypes.c_int64 * 3)(st[0], st[2], st[1])
    if nblk == 0:
        raise ValueError("attention_varlen_paged: the pool has no blocks")
    st = _varlen_strides((q, o), d)
    if st is None:
        q = q.contiguous()
        if _varlen_strides((o,), d) is None:
            # rows of no sequence keep what out holds: the kernel's output starts as a copy of it
            op = torch.empty((T, H, d), dtype=q.dtype, device=q.device)
            if out is not None:
                op.copy_(o)
        else:
            op = o
        st = _varlen_strides((q, op), d)
    else:
        op = o
    _launched(lib().fa_fwd_varlen_paged(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(op), _ptr(cu_seqlens),
                                        _ptr(block_table), _ptr(seqused_k), B, T, max_seqlen, Lk, H, Hkv, d, nblk, ps,
                                        tstride, st[0], cst, st[1], 1.0 / d ** 0.5,
                                        _lib.FA_FWD_CAUSAL if causal else 0, _DTYPES[q.dtype], _stream(q)))
    return _unpad_into(op, o, d)


@_on_tensor_device
def kv_cache_append_paged(k_new, v_new, k_cache, v_cache, cu_seqlens, max_seqlen, block_table, seqused_k):
    """Write a chunk's new K / V rows into the pages of a paged KV cache (fa_kv_append_paged), in
    place, on the current stream, with nothing read on the host.  k_new, v_new ``[T, H_kv, d]``
    (token-packed like attention_varlen's k / v: read in place under its stride rules, e.g. the K
    and V slices of a fused QKV projection; other views are copied), pools ``[num_blocks,
    page_size, H_kv, d]`` under attention_varlen_paged's rules, ``block_table`` int32 ``[B, P]``.
    ``cu_seqlens`` / ``max_seqlen`` name each sequence's new tokens and are clamped on the device
    like attention_varlen's.  ``seqused_k[b]`` is the sequence's key count AFTER the append -- pass
    the same array to attention_varlen_paged next: new token i of a sequence with len_q new tokens
    becomes logical key ``p = seqused_k[b] - len_q + i``, row ``p % page_size`` of block
    ``block_table[b, p // page_size]`` (clamped to the pool).  A token with p < 0 or p >= P *
    page_size has no page and is skipped.  Only rows that a token owns are written.

    d is any multiple of 8 up to 256, bfloat16 or float16; other head dims, float64, page sizes
    that are not multiples of 64 and pool views that cannot be addressed raise NotImplementedError."""
    for name, t in (("k_new", k_new), ("v_new", v_new), ("k_cache", k_cache), ("v_cache", v_cache),
                    ("cu_seqlens", cu_seqlens), ("block_table", block_table), ("seqused_k", seqused_k)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    for name, t in (("k_new", k_new), ("v_new", v_new)):
        if t.dim() != 3:
            raise ValueError(f"{name} must be 3-D [tokens, heads, d], got shape {tuple(t.shape)}")
    if k_cache.dim() != 4:
        raise ValueError(f"k_cache must be 4-D [num_blocks, page_size, H_kv, d], got shape {tuple(k_cache.shape)}")
    if k_new.dtype not in _DTYPES:
        raise ValueError(f"k_new dtype {k_new.dtype} unsupported (bfloat16 or float16)")
    if k_new.shape != v_new.shape:
        raise ValueError(f"k_new {tuple(k_new.shape)} and v_new {tuple(v_new.shape)} must have the same shape")
    if tuple(k_new.shape[1:]) != (k_cache.shape[2], k_cache.shape[3]):
        raise ValueError(f"k_new {tuple(k_new.shape)} and k_cache {tuple(k_cache.shape)} disagree on H_kv or d")
    if block_table.dtype != torch.int32 or block_table.dim() != 2:
        raise ValueError(f"block_table must be an int32 tensor of shape (B, pages), got {block_table.dtype} "
                         f"{tuple(block_table.shape)}")
    if seqused_k.dtype != torch.int32 or seqused_k.dim() != 1:
        raise ValueError(f"seqused_k must be an int32 tensor of shape (B,), got {seqused_k.dtype} "
                         f"{tuple(seqused_k.shape)}")
    _check_tensor("k_new", k_new, ndim=3, strided=True)
    _check_tensor("v_new", v_new, k_new.dtype, k_new.device, ndim=3, strided=True)
    B = _check_cu_seqlens(cu_seqlens, k_new.device)
    T, Hkv, d = k_new.shape
    if k_new.dtype == torch.float64:
        raise NotImplementedError("kv_cache_append_paged: float64 tensors are not supported (use bfloat16 or float16)")
    if d <= 0 or d % 8 or d > 256:
        raise NotImplementedError(f"kv_cache_append_paged: head dim d={d} is not supported (a multiple of 8 up to 256)")
    nblk, ps, _, P, tstride, cst = _paged_pool_args("kv_cache_append_paged", k_cache, v_cache, k_new.dtype,
                                                    k_new.device, block_table, seqused_k, B)
    max_seqlen = int(max_seqlen)
    if max_seqlen < 0:
        raise ValueError(f"max_seqlen={max_seqlen} must not be negative")
    if k_new.numel() == 0 or B == 0 or max_seqlen == 0 or P == 0:  # no token that could be placed
        return
    if nblk == 0:
        raise ValueError("kv_cache_append_paged: the pool has no blocks")
    st = _varlen_strides((k_new,), d) if k_new.stride() == v_new.stride() else None
    if st is None or _varlen_strides((v_new,), d) is None:
        k_new, v_new = k_new.contiguous(), v_new.contiguous()
        st = _varlen_strides((k_new,), d)
    _launched(lib().fa_kv_append_paged(_ptr(k_new), _ptr(v_new), _ptr(k_cache), _ptr(v_cache), _ptr(cu_seqlens),
                                       _ptr(block_table), _ptr(seqused_k), B, T, max_seqlen, P * ps, Hkv, d, nblk, ps,
                                       tstride, st[0], cst, _DTYPES[k_new.dtype], _stream(k_new)))


def kernel_geometry(d, dtype=torch.bfloat16):
    """(bq, bk, threads, lds_bytes) the library uses for head dim d."""
    return _lib.geometry(d, _DTYPES[dtype])
