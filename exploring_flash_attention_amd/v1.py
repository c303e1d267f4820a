"""FA-v1 fused forward -- drop-in surfaces of the reference's flash_attention_v1 family.

Reference surfaces mirrored (tyler-utah/exploring_flash_attention):

* ``flash_attention_tiled(Q, K, V, Bq=8, Bk=8) -> O``
      flash_attention_v1/numpy_basic.py:69  (host [L, d] arrays in, [L, d] out)
* ``flash_attention_tiled(Q, K, V, O, L, d, Bq=8, Bk=8)``
      flash_attention_v1/numpy_gpu_like_opt2.py:198  (flat [L*d] buffers, O written in place;
      also the signature of numpy_gpu_like.py:288 / _1D.py:320 / _opt1.py:320)
* ``flash_attention_v1(Q, K, V, O, B, H, L, d)`` and ``flash_attention_v1_opt1(...)``
      flash_attention_v1/CUDA/flash_attention_v1.h:251, flash_attention_v1_opt1.h:354
      (device [B, H, L, d] tensors, O written in place)
* ``flash_attention_v1(Q, K, V) -> O`` -- the ``naive_attention(Q, K, V)`` form
      (common/reference.py:7): NumPy [L, d] / [B, H, L, d] or torch device tensors

``Bq`` / ``Bk`` are the reference's tile sizes; they are accepted and validated (> 0) but
the gfx950 kernel uses its own tiles (128 query rows x 64 keys, see
``ops.kernel_geometry``) -- the result does not depend on them.
"""
import functools

import numpy as np
import torch

from . import _host, ops


def _check_tiles(Bq, Bk):
    assert isinstance(Bq, (int, np.integer)) and Bq > 0, "Bq must be a positive int"
    assert isinstance(Bk, (int, np.integer)) and Bk > 0, "Bk must be a positive int"


def _run_host(Q, K, V):
    Q, K, V = (np.asarray(x) for x in (Q, K, V))
    assert Q.ndim == 2 and Q.shape == K.shape == V.shape, "Q, K, V must have the same shape [L, d]"
    dt = _host.compute_dtype(Q, K, V)
    q, k, v = _host.to_device((Q, K, V), dt)
    return _host.to_host(ops.attention_v1(q, k, v), Q.dtype)


def flash_attention_tiled(Q, K, V, *args, Bq=8, Bk=8, **kw):
    """Both reference surfaces of ``flash_attention_tiled`` (see module docstring)."""
    if args or "O" in kw:  # C-style: (Q, K, V, O, L, d, Bq=8, Bk=8)
        names = ("O", "L", "d", "Bq", "Bk")
        vals = dict(zip(names, args))
        vals.update(kw)
        vals.setdefault("Bq", Bq)
        vals.setdefault("Bk", Bk)
        O, L, d = vals["O"], int(vals["L"]), int(vals["d"])
        _check_tiles(vals["Bq"], vals["Bk"])
        q2, k2, v2 = (np.asarray(x).reshape(L, d) for x in (Q, K, V))
        O[:L * d] = _run_host(q2, k2, v2).reshape(-1).astype(O.dtype, copy=False)
        return None
    if kw:
        raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
    _check_tiles(Bq, Bk)
    if _host.is_device_tensor(Q):
        if Q.dim() == 2:
            return ops.attention_v1(Q[None, None], K[None, None], V[None, None])[0, 0]
        return ops.attention_v1(Q, K, V)
    return _run_host(Q, K, V)


def flash_attention_v1(Q, K, V, O=None, B=None, H=None, L=None, d=None, causal=False):
    """``flash_attention_v1(Q, K, V) -> O`` (host or device), or the launcher form
    ``flash_attention_v1(Q, K, V, O, B, H, L, d)``: O[B,H,L,d] written in place,
    asynchronous on the current stream.

    ``causal=True`` (not in the reference): row i attends to keys 0..i, see
    ``ops.attention_v1``.  bf16 / fp16 only: host arrays other than float16 would run the
    fp64 kernels, which have no causal mode, and raise NotImplementedError.

    Grouped-query attention: ``[B, H, L, d]`` Q with ``[B, H_kv, L, d]`` K and V (H a multiple of
    H_kv) passes through to ``ops.attention_v1`` for device tensors and float16 host arrays;
    float32 / float64 host arrays raise NotImplementedError, as they do for causal."""
    if O is None:
        if not _host.is_device_tensor(Q) and np.ndim(Q) == 4 and np.ndim(K) == 4 and np.shape(Q)[1] != np.shape(K)[1] \
                and _host.compute_dtype(*(np.asarray(x) for x in (Q, K, V))) == torch.float64:
            raise NotImplementedError("grouped-query attention (GQA): float32 / float64 host arrays run the float64 "
                                      "kernels, which read one K/V head per query head (pass float16 arrays or "
                                      "bf16 / fp16 device tensors)")
        if not causal:
            return _host.run_qkv(ops.attention_v1, Q, K, V)
        if not _host.is_device_tensor(Q) and _host.compute_dtype(*(np.asarray(x) for x in (Q, K, V))) == torch.float64:
            raise NotImplementedError("causal attention: float32 / float64 host arrays run the float64 kernels, "
                                      "which have no causal mode (pass float16 arrays or bf16 / fp16 device tensors)")
        return _host.run_qkv(functools.partial(ops.attention_v1, causal=True), Q, K, V)
    assert B > 0 and H > 0 and L > 0 and d > 0, "All dimensions must be positive"
    assert tuple(Q.shape) == (B, H, L, d), f"Q shape {tuple(Q.shape)} != {(B, H, L, d)}"
    ops.attention_v1(Q, K, V, out=O, causal=causal)


flash_attention_v1_opt1 = flash_attention_v1
