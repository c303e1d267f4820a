"""Paged chunked prefill: fa_fwd_varlen_paged / ops.attention_varlen_paged (the varlen forward with
its keys in a block-table pool) and fa_kv_append_paged / ops.kv_cache_append_paged (a chunk's new
K / V into the pool's pages).

Key j of sequence b is row j % page_size of block clamp(block_table[b][j // page_size], 0,
num_blocks - 1); the sequence has clamp(seqused_k[b], 0, max_seqlen_k) keys.  The attention result is
bit for bit attention_varlen(cu_seqlens_k=, seqused_k=) on the cache gathered in table order, so
no test here needs a tolerance of its own: the fp64 comparisons use tests/test_varlen.py's GATE.

CPU part: both C entries' argument checks (no launch), the Python-side checks, and NumPy replays of
the PAGED address arithmetic of csrc/fa_fwd_kernel.hpp (the page cursor, every table read, every
K / V descriptor of whole grids) and of csrc/fa_kv_append.hip (every source and destination row).
GPU part: bitwise comparisons against the gathered call, stray-store and corrupt-array checks,
chunked prefill end to end through the append, graph replay, one softmax-weight readout.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L
from test_varlen import (DTYPES, FAKE, GUARD, IDS, KBQ, NULL, SENTINEL, Alloc, _batch, _cu_dev, _gate, bk_for,
                         varlen_ref, xcd_remap)
from test_varlen_kv import CORRUPT_SEQUSED, INT32_MAX, item_schedule, kv_ref, side_clamp

INT32_MIN = -2 ** 31
APPEND_ROWS = 32  # token rows per workgroup of the append kernel (fa_internal.hpp kAppendRows)


# ----------------------------------------------------------------------------------------
# CPU: the C entries' argument checks, the exports
# ----------------------------------------------------------------------------------------


def _fwd(fn, q=FAKE, k=FAKE, v=FAKE, o=FAKE, cu=FAKE, tbl=FAKE, su=FAKE, B=2, T=300, msl=200, mslk=400, H=4, Hkv=2,
         d=128, nb=16, ps=64, ts=7, qs=None, cs=None, os_=None, scale=0.1, flags=0, dtype=L.FA_DTYPE_BF16):
    return fn(q, k, v, o, cu, tbl, su, B, T, msl, mslk, H, Hkv, d, nb, ps, ts, qs, cs, os_, scale, flags, dtype, NULL)


def _app(fn, kn=FAKE, vn=FAKE, k=FAKE, v=FAKE, cu=FAKE, tbl=FAKE, su=FAKE, B=2, T=300, msl=200, mslk=400, Hkv=2, d=128,
         nb=16, ps=64, ts=7, ns=None, cs=None, dtype=L.FA_DTYPE_BF16):
    return fn(kn, vn, k, v, cu, tbl, su, B, T, msl, mslk, Hkv, d, nb, ps, ts, ns, cs, dtype, NULL)


def _shared_entry_checks(call, err, tensors):
    """The checks both entries make the same way."""
    for name in tensors:
        assert call(**{name: NULL}) == L.FA_ERR_INVALID_ARG and b"null" in err()
        assert call(**{name: ctypes.c_void_p(0x10008)}) == L.FA_ERR_INVALID_ARG and b"aligned" in err()
    for name, word in (("cu", b"cu_seqlens"), ("tbl", b"block_table"), ("su", b"seqused_k")):
        assert call(**{name: NULL}) == L.FA_ERR_INVALID_ARG and word in err()       # seqused_k is required here
        assert call(**{name: ctypes.c_void_p(0x10002)}) == L.FA_ERR_INVALID_ARG and word in err()
    for B in (0, -1):
        assert call(B=B) == L.FA_ERR_INVALID_ARG and b"B=" in err()
    for msl in (0, -5):
        assert call(msl=msl) == L.FA_ERR_INVALID_ARG and b"max_seqlen=" in err()
    for mslk in (0, -5):
        assert call(mslk=mslk) == L.FA_ERR_INVALID_ARG and b"max_seqlen_k" in err()
    assert call(T=-1) == L.FA_ERR_INVALID_ARG and b"total_tokens=" in err()
    assert call(T=1 << 31) == L.FA_ERR_UNSUPPORTED and b"total_tokens=" in err()
    assert call(dtype=L.FA_DTYPE_FP64) == L.FA_ERR_UNSUPPORTED and b"FP64" in err()
    assert call(dtype=L.FA_DTYPE_FP32) == L.FA_ERR_UNSUPPORTED and b"dtype" in err()
    for nb in (0, -3, 1 << 31):
        assert call(nb=nb) == L.FA_ERR_INVALID_ARG and b"num_blocks" in err()
    for ps in (0, -64):
        assert call(ps=ps) == L.FA_ERR_INVALID_ARG and b"page_size" in err()
    for ps in (16, 32, 96, 100):
        assert call(ps=ps, ts=64) == L.FA_ERR_UNSUPPORTED and b"page_size" in err()
    assert call(mslk=449, ts=7) == L.FA_ERR_INVALID_ARG and b"table_stride" in err()    # 449 keys: 8 pages of 64
    assert call(mslk=448, ts=7) == L.FA_OK or b"table_stride" not in err()
    assert call(ts=0) == L.FA_ERR_INVALID_ARG and b"table_stride" in err()
    S3 = ctypes.c_int64 * 3
    for bad in ((16388, 128, 256), (16384, 4, 256), (16384, 128, 0), (-8, 128, 256)):
        assert call(cs=S3(*bad)) == L.FA_ERR_INVALID_ARG and b"cache_strides" in err()
    assert call(cs=S3(16384, 128, 64)) == L.FA_ERR_INVALID_ARG and b"row stride" in err()
    assert call(cs=S3(1 << 30, 128, (1 << 20) + 8)) == L.FA_ERR_UNSUPPORTED and b"row stride" in err()


def test_varlen_paged_entry_argument_checks():
    lib = L.lib()
    fn, err = lib.fa_fwd_varlen_paged, lib.fa_last_error
    call = functools.partial(_fwd, fn)
    _shared_entry_checks(call, err, ("q", "k", "v", "o"))
    for Hkv in (3, 0, 8, -1):
        assert call(Hkv=Hkv) == L.FA_ERR_INVALID_ARG and b"H_kv" in err()
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == L.FA_ERR_INVALID_ARG and b"flags" in err()
    for d in (96, 384, 512):
        assert call(d=d) == L.FA_ERR_UNSUPPORTED and f"d={d}".encode() in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(scale=bad) == L.FA_ERR_INVALID_ARG and b"softmax_scale" in err()
    assert call(B=1 << 20, H=1 << 10, Hkv=1 << 10, T=1 << 30, msl=1 << 10) == L.FA_ERR_UNSUPPORTED and b"grid" in err()
    S2 = ctypes.c_int64 * 2
    for which in ("qs", "os_"):
        for bad in ((1028, 128), (1024, 4), (0, 128), (1024, -8)):
            assert call(**{which: S2(*bad)}) == L.FA_ERR_INVALID_ARG and b"stride" in err()
        assert call(**{which: S2(64, 128)}) == L.FA_ERR_INVALID_ARG and b"token stride" in err()
        assert call(**{which: S2((1 << 20) + 8, 128)}) == L.FA_ERR_UNSUPPORTED and b"token stride" in err()
    # no query tokens: FA_OK, nothing launched (the pointers are fakes)
    assert call(T=0) == L.FA_OK and lib.fa_last_kernels() == b""


def test_kv_append_entry_argument_checks():
    lib = L.lib()
    fn, err = lib.fa_kv_append_paged, lib.fa_last_error
    call = functools.partial(_app, fn)
    _shared_entry_checks(call, err, ("kn", "vn", "k", "v"))
    for Hkv in (0, -1):
        assert call(Hkv=Hkv) == L.FA_ERR_INVALID_ARG and b"H_kv" in err()
    for d in (0, -8):
        assert call(d=d) == L.FA_ERR_INVALID_ARG and b"d=" in err()
    for d in (4, 100, 264, 512):
        assert call(d=d) == L.FA_ERR_UNSUPPORTED and b"head dim" in err() and f"d={d}".encode() in err()
    assert call(B=1 << 20, Hkv=1 << 10, T=1 << 30, msl=1 << 10) == L.FA_ERR_UNSUPPORTED and b"grid" in err()
    S2 = ctypes.c_int64 * 2
    for bad in ((260, 128), (256, 4), (0, 128), (256, -8)):
        assert call(ns=S2(*bad)) == L.FA_ERR_INVALID_ARG and b"stride" in err()
    assert call(ns=S2(64, 128)) == L.FA_ERR_INVALID_ARG and b"token stride" in err()
    assert call(ns=S2((1 << 20) + 8, 128)) == L.FA_ERR_UNSUPPORTED and b"token stride" in err()
    assert call(T=0) == L.FA_OK and lib.fa_last_kernels() == b""


def test_paged_entries_are_declared_and_exported():
    sig = L.SIGNATURES
    assert len(sig["fa_fwd_varlen_paged"][1]) == 24 and len(sig["fa_kv_append_paged"][1]) == 20
    assert len(sig["fa_fwd_varlen_kv"][1]) == 22 and len(sig["fa_fwd_decode_paged"][1]) == 23  # unchanged
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fa_mi355x.h")) as f:
        text = f.read()
    assert "int fa_fwd_varlen_paged(" in text and "int fa_kv_append_paged(" in text
    assert "#define FA_MI355X_VERSION_MINOR 4" in text and L.lib().fa_version() == 0x000400
    assert hasattr(L.lib(), "fa_fwd_varlen_paged") and hasattr(L.lib(), "fa_kv_append_paged")
    import exploring_flash_attention_amd as pkg
    assert pkg.attention_varlen_paged is pkg.ops.attention_varlen_paged
    assert pkg.kv_cache_append_paged is pkg.ops.kv_cache_append_paged


def test_paged_python_side_checks():
    """Everything the operators reject before a tensor's device matters, and the device check."""
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q, pool = torch.zeros(8, 4, 64, dtype=bf), torch.zeros(6, 64, 2, 64, dtype=bf)
    cu, tbl, su = (torch.zeros(n, dtype=torch.int32) for n in (3, 4, 2))
    tbl = tbl.view(2, 2)
    att, app = ops.attention_varlen_paged, ops.kv_cache_append_paged
    kn = torch.zeros(8, 2, 64, dtype=bf)
    with pytest.raises(TypeError, match="block_table"):
        att(q, pool, pool, cu, 8, [[0]], su)
    with pytest.raises(TypeError, match="k_new"):
        app(None, kn, pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="3-D"):
        att(q[0], pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="4-D"):
        att(q, pool[0], pool[0], cu, 8, tbl, su)
    with pytest.raises(ValueError, match="3-D"):
        app(kn[0], kn[0], pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="disagree on d"):
        att(torch.zeros(8, 4, 32, dtype=bf), pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="H_kv or d"):
        app(torch.zeros(8, 4, 64, dtype=bf), torch.zeros(8, 4, 64, dtype=bf), pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="same shape"):
        app(kn, kn[:7], pool, pool, cu, 8, tbl, su)
    with pytest.raises(ValueError, match="dtype"):
        att(q.float(), pool, pool, cu, 8, tbl, su)
    for fn, first in ((att, q), (app, kn)):
        args = (first, kn) if fn is app else (first,)
        with pytest.raises(ValueError, match="block_table"):
            fn(*args, pool, pool, cu, 8, tbl.long(), su)
        with pytest.raises(ValueError, match="block_table"):
            fn(*args, pool, pool, cu, 8, tbl[0], su)
        with pytest.raises(ValueError, match="seqused_k"):
            fn(*args, pool, pool, cu, 8, tbl, su.long())
        with pytest.raises(ValueError, match="seqused_k"):
            fn(*args, pool, pool, cu, 8, tbl, su.view(1, 2))
        with pytest.raises(ValueError, match="ROCm device"):  # host tensors: no CPU fallback
            fn(*args, pool, pool, cu, 8, tbl, su)


@pytest.mark.gpu
def test_paged_python_side_checks_on_the_device(gpu):
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    z = functools.partial(torch.zeros, device=gpu)
    q, kn, pool = z(8, 4, 64, dtype=bf), z(8, 2, 64, dtype=bf), z(6, 64, 2, 64, dtype=bf)
    cu, su, tbl = _cu_dev([0, 5, 8], gpu), _cu_dev([5, 3], gpu), z(2, 2, dtype=torch.int32)
    att, app = ops.attention_varlen_paged, ops.kv_cache_append_paged
    for fn, args in ((att, (q,)), (app, (kn, kn))):
        with pytest.raises(ValueError, match="block_table"):       # B rows
            fn(*args, pool, pool, cu, 8, z(3, 2, dtype=torch.int32), su)
        with pytest.raises(ValueError, match="contiguous"):        # last dim strided
            fn(*args, pool, pool, cu, 8, z(2, 4, dtype=torch.int32)[:, ::2], su)
        with pytest.raises(ValueError, match="apart"):             # overlapping rows
            fn(*args, pool, pool, cu, 8, z(4, dtype=torch.int32).as_strided((2, 2), (1, 1)), su)
        with pytest.raises(ValueError, match="seqused_k"):
            fn(*args, pool, pool, cu, 8, tbl, _cu_dev([5, 3, 1], gpu))
        with pytest.raises(ValueError, match="same shape"):
            fn(*args, pool, pool[:5], cu, 8, tbl, su)
        with pytest.raises(ValueError, match="v_cache"):
            fn(*args, pool, pool.half(), cu, 8, tbl, su)
        with pytest.raises(ValueError, match="cu_seqlens"):
            fn(*args, pool, pool, cu.long(), 8, tbl, su)
        with pytest.raises(ValueError, match="block_table"):       # a host table
            fn(*args, pool, pool, cu, 8, tbl.cpu(), su)
        # NotImplementedError: views of the pool that cannot be addressed in place, small pages
        with pytest.raises(NotImplementedError, match="in place"):
            fn(*args, z(6, 64, 2, 128, dtype=bf)[..., ::2], z(6, 64, 2, 128, dtype=bf)[..., ::2], cu, 8, tbl, su)
        with pytest.raises(NotImplementedError, match="in place"):  # k and v strided differently
            fn(*args, pool, z(6, 2, 64, 64, dtype=bf).transpose(1, 2), cu, 8, tbl, su)
        with pytest.raises(NotImplementedError, match="in place"):  # a misaligned base
            fn(*args, z(6 * 64 * 2 * 64 + 4, dtype=bf)[4:].view(6, 64, 2, 64), pool, cu, 8, tbl, su)
        for ps in (16, 32, 96):
            with pytest.raises(NotImplementedError, match="page_size"):
                fn(*args, z(6, ps, 2, 64, dtype=bf), z(6, ps, 2, 64, dtype=bf), cu, 8, tbl, su)
    with pytest.raises(ValueError, match="max_seqlen_k"):
        att(q, pool, pool, cu, 8, tbl, su, max_seqlen_k=129)       # P * page_size = 128
    with pytest.raises(ValueError, match="H_kv"):
        att(z(8, 3, 64, dtype=bf), pool, pool, cu, 8, tbl, su)
    for d in (16, 80, 96):
        with pytest.raises(NotImplementedError, match="head dim"):
            att(z(8, 4, d, dtype=bf), z(6, 64, 2, d, dtype=bf), z(6, 64, 2, d, dtype=bf), cu, 8, tbl, su)
    with pytest.raises(NotImplementedError, match="head dim"):
        att(z(8, 1, 384, dtype=bf), z(6, 64, 1, 384, dtype=bf), z(6, 64, 1, 384, dtype=bf), cu, 8, tbl, su)
    with pytest.raises(NotImplementedError, match="float64"):
        att(z(8, 4, 64, dtype=torch.float64), z(6, 64, 2, 64, dtype=torch.float64), z(6, 64, 2, 64, dtype=torch.float64),
            cu, 8, tbl, su)
    with pytest.raises(NotImplementedError, match="float64"):
        app(z(8, 2, 64, dtype=torch.float64), z(8, 2, 64, dtype=torch.float64), z(6, 64, 2, 64, dtype=torch.float64),
            z(6, 64, 2, 64, dtype=torch.float64), cu, 8, tbl, su)
    with pytest.raises(NotImplementedError, match="head dim"):
        app(z(8, 2, 12, dtype=bf), z(8, 2, 12, dtype=bf), z(6, 64, 2, 12, dtype=bf), z(6, 64, 2, 12, dtype=bf), cu, 8, tbl, su)
    # nothing to launch
    with ops.launched_kernels() as kl:
        assert tuple(att(q[:0], pool, pool, _cu_dev([0, 0, 0], gpu), 8, tbl, su).shape) == (0, 4, 64)
        out = torch.full_like(q, SENTINEL)
        att(q, pool, pool, _cu_dev([0], gpu), 8, z(0, 2, dtype=torch.int32), z(0, dtype=torch.int32), out=out)  # B = 0
        att(q, pool, pool, cu, 0, tbl, su, out=out)
        assert (out == SENTINEL).all()
        app(kn[:0], kn[:0], pool, pool, _cu_dev([0, 0, 0], gpu), 8, tbl, su)
        app(kn, kn, pool, pool, cu, 0, tbl, su)
    assert kl == []
    # max_seqlen_k = 0: every owned row is zeros, the others are kept
    out = torch.full_like(q, SENTINEL)
    att(q, pool, pool, _cu_dev([0, 5, 6], gpu), 8, tbl, su, max_seqlen_k=0, out=out)
    assert (out[:6] == 0).all() and (out[6:] == SENTINEL).all()


# ----------------------------------------------------------------------------------------
# CPU: replay of the PAGED variant (csrc/fa_fwd_kernel.hpp) -- cursor, table reads, descriptors
# ----------------------------------------------------------------------------------------


def clamp_entry(e, nb):
    return min(max(int(e), 0), nb - 1)


def replay_paged(cu_q, seqused, table, Tq, msl_q, msl_k, H, Hkv, D, causal, ps, nb, tstride, cst, pool_alloc,
                 clamp=True):
    """Replay the key side of one fa_fwd_varlen_paged launch.  table: the flat int32 table the
    kernel's pointer names (row b at b * tstride); cst: {block, head, row} element strides of the
    pool.  Walks every running work item's page cursor as the kernel does (three look-ups in the
    prologue, one per step) and asserts: the cursor names tile t's page and row; every table read is
    inside the table and at a page that holds a key below kv_end; every non-empty descriptor lies in
    the pool, inside one block, and covers only rows of keys below len_k.  Returns (table reads as
    (b, page) pairs, descriptors as (b, hkv, tile, block, first row, rows))."""
    cu_q = np.asarray(cu_q, np.int64)
    B = len(cu_q) - 1
    nqt = (min(msl_q, Tq) + KBQ - 1) // KBQ
    G, bk, ROWB = H // Hkv, bk_for(D), 2 * D
    assert ps % 64 == 0 and ps % bk == 0 and tstride >= (msl_k + ps - 1) // ps
    nblk = B * H * nqt
    blk = np.arange(nblk, dtype=np.int64)
    w = xcd_remap(blk, nblk)
    if causal:
        g, rest = w % G, w // G
        qt, bh = nqt - 1 - rest % nqt, (rest // nqt) * G + g
    else:
        qt, bh = w % nqt, w // nqt
    b, h = bh // H, bh % H
    assert np.array_equal(np.sort((b * H + h) * nqt + qt), blk), "decode is not a bijection"
    _, nq = side_clamp(cu_q, Tq, msl_q)
    nk = np.clip(np.asarray(seqused, np.int64), 0, msl_k)
    bs, hs, rs = cst
    krb = 2 * rs
    reads, descs = set(), []
    for i in np.nonzero(qt * KBQ < nq[b])[0]:
        bi, hkv, qti = int(b[i]), int(h[i]) // G, int(qt[i])
        lq, lk = int(nq[bi]), int(nk[bi])
        nkv, ntiles, _, _ = item_schedule(qti, lq, lk, bk, causal)
        if nkv <= 0:
            continue  # the zero-store exit: before the cursor exists
        pg_tiles, pg_last = ps // bk, (nkv - 1) // ps
        state = {"page": 0, "in": 0}

        def paged_next():
            page = min(state["page"], pg_last)
            assert 0 <= bi * tstride + page < len(table), "a table read outside the table"
            assert page * ps < nkv, "a table read at a page without a key below kv_end"
            reads.add((bi, page))
            e, row = int(table[bi * tstride + page]), state["in"] * bk
            wrap = state["in"] + 1 == pg_tiles
            state["in"] = 0 if wrap else state["in"] + 1
            state["page"] += 1 if wrap else 0
            return e, row

        looked = [paged_next() for _ in range(3)]            # the prologue: tiles 0, 1, 2
        for _ in range(ntiles):                              # step t looks tile t + 3 up
            looked.append(paged_next())
        for t in range(ntiles + 2):                          # K(t) for t < ntiles + 2 at most, V(t) for t < ntiles
            vld = min(max(nkv - t * bk, 0), bk)
            if vld == 0:
                assert t >= ntiles                           # an empty descriptor: nothing is read
                continue
            e, row = looked[t]
            assert t // pg_tiles <= pg_last and e == int(table[bi * tstride + t // pg_tiles]), "the cursor lost its page"
            assert row == (t % pg_tiles) * bk, "the cursor lost its row"
            blk_i = clamp_entry(e, nb) if clamp else e
            base, length = 2 * (blk_i * bs + hkv * hs + row * rs), (vld - 1) * krb + ROWB
            pool_alloc.check(base, length, f"K/V tile {t} of sequence {bi}")
            assert 2 * blk_i * bs <= base and base + length <= 2 * (blk_i + 1) * bs, "a descriptor leaves its block"
            assert row + vld <= ps and t * bk + vld <= lk, "a descriptor covers rows past len_k or the page"
            descs.append((bi, hkv, t, blk_i, row, vld))
    return reads, descs


LENS_Q, LENS_K = (130, 1, 64, 50, 129), (450, 257, 64, 0, 100)
MSL_Q = 130


def _table_for(lens_k, ps, P, nb, seed=0, fill=-1, tstride=None):
    """Pages handed out in shuffled order from a pool with spare blocks; the entries past each
    sequence's used pages hold `fill`.  Returns the flat table (row stride tstride)."""
    B, tstride = len(lens_k), P if tstride is None else tstride
    perm = np.random.default_rng(seed).permutation(nb)
    tbl = np.full((B - 1) * tstride + P, fill, np.int64)
    n = 0
    for b, lk in enumerate(lens_k):
        for p in range((lk + ps - 1) // ps):
            tbl[b * tstride + p] = perm[n]
            n += 1
    assert n <= nb
    return tbl


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("ps", (64, 128, 192))
@pytest.mark.parametrize("D", (64, 128, 256))   # kBK 64, 64, 32
def test_replay_paged_whole_grids(D, ps, causal):
    H, Hkv = 4, 2
    P = (max(LENS_K) + ps - 1) // ps
    nb = len(LENS_K) * P + 3
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)])
    Tq = int(cu_q[-1]) + GUARD
    for tstride in (P, P + 5):                              # a table view with a row stride above P
        for layout in ("[nb, ps, Hkv, d]", "[nb, Hkv, ps, d]"):
            cst = (ps * Hkv * D, D, Hkv * D) if layout[5] == "p" else (Hkv * ps * D, ps * D, D)
            table = _table_for(LENS_K, ps, P, nb, fill=INT32_MIN, tstride=tstride)
            reads, descs = replay_paged(cu_q, LENS_K, table, Tq, MSL_Q, P * ps, H, Hkv, D, causal, ps, nb, tstride, cst,
                                        Alloc("pool", 2 * nb * ps * Hkv * D))
            # exactly the used pages of the keys some query tile walks, never an unused entry
            assert all(table[bi * tstride + p] >= 0 for bi, p in reads)
            if not causal:
                want = {(bi, p) for bi, (lq, lk) in enumerate(zip(LENS_Q, LENS_K)) if lq and lk
                        for p in range((lk + ps - 1) // ps)}
                assert reads == want
            # every key below kv_end of every item is covered once per (item, tile)
            assert descs and all(rows > 0 for *_, rows in descs)
            assert {d_[0] for d_ in descs} == {0, 1, 2, 4}     # sequence 3 has no key


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_replay_paged_cursor_on_long_sequences(causal):
    """Many pages and more than one query tile: the cursor against the closed form, at both tile sizes."""
    for D, ps in ((128, 64), (256, 64), (128, 192), (256, 192)):
        lens_q, lens_k = (300, 5), (1500, 1000)
        P = (1500 + ps - 1) // ps
        nb = 2 * P
        table = _table_for(lens_k, ps, P, nb, seed=3)
        reads, descs = replay_paged([0, 300, 305], lens_k, table, 305, 300, P * ps, 4, 1, D, causal, ps, nb, P,
                                    (ps * D, D, D), Alloc("pool", 2 * nb * ps * D))
        assert max(p for _, p in reads) == (1500 - 1) // ps


CORRUPT_ENTRIES = (-1, "num_blocks", INT32_MAX, INT32_MIN)


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("entry", CORRUPT_ENTRIES)
def test_replay_paged_corrupt_table_entries_are_clamped(entry, causal):
    D, ps, H, Hkv = 128, 64, 4, 2
    P = (max(LENS_K) + ps - 1) // ps
    nb = len(LENS_K) * P + 3
    table = _table_for(LENS_K, ps, P, nb)
    table[table >= 0] = nb if entry == "num_blocks" else entry        # every used position
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)])
    _, descs = replay_paged(cu_q, LENS_K, table, int(cu_q[-1]), MSL_Q, P * ps, H, Hkv, D, causal, ps, nb, P,
                            (ps * Hkv * D, D, Hkv * D), Alloc("pool", 2 * nb * ps * Hkv * D))
    assert {d_[3] for d_ in descs} == {0 if entry in (-1, INT32_MIN) else nb - 1}


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("name", sorted(CORRUPT_SEQUSED))
def test_replay_paged_corrupt_seqused_is_clamped(name, causal):
    D, ps, H, Hkv, P = 128, 64, 4, 2, 8
    nb = 5 * P
    table = np.random.default_rng(1).permutation(nb).astype(np.int64)   # every entry valid: huge lengths read all
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)])
    for msl_k in (P * ps, 257):
        _, descs = replay_paged(cu_q, CORRUPT_SEQUSED[name], table, int(cu_q[-1]), MSL_Q, msl_k, H, Hkv, D, causal, ps,
                                nb, P, (ps * Hkv * D, D, Hkv * D), Alloc("pool", 2 * nb * ps * Hkv * D))
        assert all(t * 64 + rows <= msl_k for _, _, t, _, _, rows in descs)


def test_replay_paged_catches_a_missing_entry_clamp():
    D, ps, H, Hkv = 128, 64, 4, 2
    P = (max(LENS_K) + ps - 1) // ps
    nb = len(LENS_K) * P + 3
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)])
    for entry in (-1, nb, INT32_MAX, INT32_MIN):
        table = _table_for(LENS_K, ps, P, nb)
        table[table >= 0] = entry
        with pytest.raises(AssertionError, match="leaves pool"):
            replay_paged(cu_q, LENS_K, table, int(cu_q[-1]), MSL_Q, P * ps, H, Hkv, D, False, ps, nb, P,
                         (ps * Hkv * D, D, Hkv * D), Alloc("pool", 2 * nb * ps * Hkv * D), clamp=False)


# ----------------------------------------------------------------------------------------
# CPU: replay of the append kernel (csrc/fa_kv_append.hip)
# ----------------------------------------------------------------------------------------


def replay_append(cu, seqused, table, T, msl, msl_k, Hkv, d, ps, nb, tstride, nst, cst, new_alloc, pool_alloc):
    """Replay one fa_kv_append_paged launch: every (sequence, row block, K/V head) work item and every
    16-byte piece.  Asserts that every source lies in k_new, every destination in the pool and
    every table read in the table.  Returns {(block, head, row in page): (token row, head)}."""
    cu = np.asarray(cu, np.int64)
    B = len(cu) - 1
    st, nq = side_clamp(cu, T, msl)
    nrb = (min(msl, T) + APPEND_ROWS - 1) // APPEND_ROWS
    assert tstride >= (msl_k + ps - 1) // ps
    written = {}
    for item in range(B * nrb * Hkv):
        hkv, rest = item % Hkv, item // Hkv
        rb, bi = rest % nrb, rest // nrb
        lq, row0 = int(nq[bi]), rb * APPEND_ROWS
        if row0 >= lq:
            continue
        p0 = int(seqused[bi]) - lq
        for r in range(min(lq - row0, APPEND_ROWS)):
            i = row0 + r
            p = p0 + i
            if p < 0 or p >= msl_k:
                continue
            page, inp = p // ps, p % ps
            assert 0 <= bi * tstride + page < len(table), "a table read outside the table"
            blk = clamp_entry(table[bi * tstride + page], nb)
            for c in range(d // 8):
                new_alloc.check(2 * ((int(st[bi]) + i) * nst[0] + hkv * nst[1] + 8 * c), 16, "source piece")
                pool_alloc.check(2 * (blk * cst[0] + hkv * cst[1] + inp * cst[2] + 8 * c), 16, "destination piece")
            key = (blk, hkv, inp)
            assert key not in written or written[key][0] // 10 ** 9 != bi, "one sequence writes a row twice"
            written[key] = (int(st[bi]) + i, hkv)
    return written


def test_replay_append_destinations():
    Hkv, d, ps, P = 2, 128, 64, 8
    nb = 5 * P + 3
    lens_new, after = (130, 1, 64, 0, 33), (450, 257, 64, 17, 100)      # a straddled page, len_q = 0, old keys kept
    cu = np.concatenate([[0], np.cumsum(lens_new)])
    T = int(cu[-1]) + GUARD
    for tstride in (P, P + 3):
        table = _table_for(after, ps, P, nb, tstride=tstride)
        for nst, new_bytes in (((Hkv * d, d), 2 * T * Hkv * d), ((8 * d, d), 2 * T * 8 * d)):   # packed; a QKV slice
            written = replay_append(cu, after, table, T, 130, P * ps, Hkv, d, ps, nb, tstride, nst,
                                    (ps * Hkv * d, d, Hkv * d), Alloc("k_new", new_bytes - 2 * (nst[0] - Hkv * d)),
                                    Alloc("pool", 2 * nb * ps * Hkv * d))
            want = {}
            for b, (n, lk) in enumerate(zip(lens_new, after)):
                for i in range(n):
                    p = lk - n + i
                    for hkv in range(Hkv):
                        want[(int(table[b * tstride + p // ps]), hkv, p % ps)] = (int(cu[b]) + i, hkv)
            assert written == want and len(want) == Hkv * sum(lens_new)   # rows of no token are not written


def test_replay_append_skips_what_has_no_page():
    """p < 0 (more new tokens than keys) and p past the table: skipped, whatever seqused_k holds."""
    Hkv, d, ps, P = 1, 64, 64, 2
    nb = 6
    table = np.array([0, 1, 2, 3, 4, 5], np.int64)
    cu = [0, 40, 80, 120]
    args = (3 * 40, 40, P * ps, Hkv, d, ps, nb, P, (d, d), (ps * d, d, d), Alloc("k_new", 2 * 120 * d),
            Alloc("pool", 2 * nb * ps * d))
    w = replay_append(cu, [10, P * ps + 15, 40], table, *args)
    rows = {b: sorted(r for (blk, _, r) in w if blk // P == b) for b in range(3)}
    assert rows[0] == list(range(10))                                 # tokens 30..39 -> keys 0..9; 0..29 have p < 0
    assert len(rows[1]) == 25 and max(rows[1]) == ps - 1              # keys 103..127; 128..142 lie past the table
    assert rows[2] == list(range(40))
    for su in ([-5, INT32_MIN, 0], [INT32_MAX, 10 ** 9, P * ps + 40]):
        assert replay_append(cu, su, table, *args) == {}
    # corrupt table entries are clamped into the pool; a corrupt cu_seqlens stays inside k_new
    replay_append(cu, [40, 40, 40], np.array([-1, nb, INT32_MAX, INT32_MIN, 7, -7], np.int64), *args)
    for bad in ([0, 500, -3, 120], [-40, 10 ** 9, 0, 0], [120, 80, 40, 0]):
        replay_append(bad, [40, 40, 40], table, *args)


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


def _nan_eq(a, b):
    """Bit-for-bit equality of 16-bit tensors that may hold NaN."""
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _scatter(packed, lens_k, ps, P, nb, table, pool=None):
    """packed [sum lens_k, H_kv, d] -> (pool [nb, ps, H_kv, d], gathered [B * P * ps, H_kv, d]): unused
    blocks and the tail of every last page hold NaN in both."""
    Hkv, d = packed.shape[1:]
    B, Lg = len(lens_k), P * ps
    gathered = torch.full((B * Lg, Hkv, d), float("nan"), dtype=packed.dtype)
    pool = torch.full((nb, ps, Hkv, d), float("nan"), dtype=packed.dtype) if pool is None else pool
    s = 0
    for b, lk in enumerate(lens_k):
        gathered[b * Lg:b * Lg + lk] = packed[s:s + lk]
        s += lk
        for p in range((lk + ps - 1) // ps):
            pool[int(table[b * P + p])] = gathered[b * Lg + p * ps:b * Lg + (p + 1) * ps]
    return pool, gathered


@functools.lru_cache(maxsize=None)
def _paged_batch(d, H, Hkv, dtype, ps, seed=0):
    """The module's batch (host, storage-rounded): q with GUARD rows, the keys packed, scattered into
    shuffled pages and gathered in table order; the table's unused entries are -1."""
    g = torch.Generator().manual_seed(500 + seed)
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)]).astype(np.int64)
    q = torch.randn(int(cu_q[-1]) + GUARD, H, d, generator=g).to(dtype)
    k, v = (torch.randn(sum(LENS_K), Hkv, d, generator=g).to(dtype) for _ in range(2))
    P = (max(LENS_K) + ps - 1) // ps
    nb = len(LENS_K) * P + 3
    table = _table_for(LENS_K, ps, P, nb, seed=seed)
    (kp, kg), (vp, vg) = _scatter(k, LENS_K, ps, P, nb, table), _scatter(v, LENS_K, ps, P, nb, table)
    return q, k, v, cu_q, kp, vp, kg, vg, torch.from_numpy(table).to(torch.int32).view(len(LENS_K), P), P


def _gathered_call(ops, q, kg, vg, cu_q, P, ps, causal, gpu, su=LENS_K, msl_k=None, out=None):
    B, Lg = len(cu_q) - 1, P * ps
    return ops.attention_varlen(q, kg, vg, cu_q, MSL_Q, causal=causal, out=out,
                                cu_seqlens_k=_cu_dev(np.arange(B + 1) * Lg, gpu),
                                max_seqlen_k=Lg if msl_k is None else msl_k, seqused_k=_cu_dev(su, gpu))


def _label(causal, gqa):
    return "fa_fwd_kernel<final, varlen, paged" + (", causal" if causal else "") + (", gqa" if gqa else "") + ">"


BITWISE_CASES = ([(d, 64, dt, 2) for d in (32, 64, 128, 256) for dt in DTYPES]
                 + [(d, ps, torch.bfloat16, 2) for d in (128, 256) for ps in (128, 192)] + [(128, 64, torch.bfloat16, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d,ps,dtype,Hkv", BITWISE_CASES,
                         ids=[f"d{d}-ps{ps}-{IDS[dt]}-Hkv{hk}" for d, ps, dt, hk in BITWISE_CASES])
def test_varlen_paged_is_bitwise_the_gathered_call(gpu, d, ps, dtype, Hkv, causal):
    from exploring_flash_attention_amd import ops
    H = 4
    q, k, v, cu_q, kp, vp, kg, vg, table, P = _paged_batch(d, H, Hkv, dtype, ps)
    qd, cud, su = q.to(gpu), _cu_dev(cu_q, gpu), _cu_dev(LENS_K, gpu)
    want = _gathered_call(ops, qd, kg.to(gpu), vg.to(gpu), cud, P, ps, causal, gpu,
                          out=torch.full(q.shape, SENTINEL, dtype=dtype, device=gpu))
    out = torch.full(q.shape, SENTINEL, dtype=dtype, device=gpu)
    with ops.launched_kernels() as kl:
        got = ops.attention_varlen_paged(qd, kp.to(gpu), vp.to(gpu), cud, MSL_Q, table.to(gpu), su, causal=causal, out=out)
    assert got is out
    assert kl == [f"{_label(causal, Hkv < H)} [grid {len(LENS_Q) * H * 2}]"], kl
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert (got[-GUARD:] == SENTINEL).all() and (got[:-GUARD] != SENTINEL).all()
    assert (got[int(cu_q[3]):int(cu_q[4])] == 0).all()                 # the sequence without keys
    if d == 128 and causal:
        ref, owned = kv_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu_q, MSL_Q,
                            np.concatenate([[0], np.cumsum(LENS_K)]), max(LENS_K), True)
        assert int((owned & (ref == 0).all(axis=(1, 2))).sum()) == 50 + 29   # len_k = 0; rows 0-28 of (129, 100)
        _gate(got.cpu()[torch.from_numpy(owned.copy())], ref[owned], dtype, f"paged d=128 ps={ps} {IDS[dtype]} Hkv={Hkv}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_paged_reads_pool_views_in_place(gpu, causal, monkeypatch):
    """A [num_blocks, H_kv, page_size, d] pool through transpose(1, 2) and a table view with a row
    stride above P: the views' own pointers and strides reach the library, the results are bitwise
    the contiguous pool's."""
    from exploring_flash_attention_amd import ops
    d, H, Hkv, ps, dtype = 128, 4, 2, 128, torch.bfloat16
    q, _, _, cu_q, kp, vp, _, _, table, P = _paged_batch(d, H, Hkv, dtype, ps)
    qd, cud, su = q.to(gpu), _cu_dev(cu_q, gpu), _cu_dev(LENS_K, gpu)
    want = ops.attention_varlen_paged(qd, kp.to(gpu), vp.to(gpu), cud, MSL_Q, table.to(gpu), su, causal=causal)
    kt, vt = (t.transpose(1, 2).contiguous().to(gpu).transpose(1, 2) for t in (kp, vp))     # [nb, Hkv, ps, d] storage
    wide = torch.full((len(LENS_K), P + 5), -1, dtype=torch.int32, device=gpu)
    wide[:, :P] = table.to(gpu)
    tv = wide[:, :P]
    assert not kt.is_contiguous() and not tv.is_contiguous()
    handle = L.lib()
    real, seen = handle.fa_fwd_varlen_paged, []

    def spy(*a):
        seen.append([x.value for x in a[:7]] + [a[14], a[15], a[16]] + [list(a[18])])
        return real(*a)

    monkeypatch.setattr(handle, "fa_fwd_varlen_paged", spy)
    out = torch.empty_like(qd)
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    got = ops.attention_varlen_paged(qd, kt, vt, cud, MSL_Q, tv, su, causal=causal, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before, "the call allocated device memory (a copy?)"
    assert seen == [[qd.data_ptr(), kt.data_ptr(), vt.data_ptr(), out.data_ptr(), cud.data_ptr(), tv.data_ptr(),
                     su.data_ptr(), kp.shape[0], ps, P + 5, [Hkv * ps * d, ps * d, d]]], seen
    assert torch.equal(got[:-GUARD], want[:-GUARD])


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128))
def test_varlen_paged_no_stray_stores(gpu, d, causal):
    """max_seqlen = 128 and max_seqlen_k = 100 cut the sequences: rows of no sequence keep the
    sentinel, and the pool is never written."""
    from exploring_flash_attention_amd import ops
    H, Hkv, ps, dtype = 4, 2, 64, torch.bfloat16
    q, k, v, cu_q, kp, vp, kg, vg, table, P = _paged_batch(d, H, Hkv, dtype, ps)
    qd, kpd, vpd, cud, su, td = q.to(gpu), kp.to(gpu), vp.to(gpu), _cu_dev(cu_q, gpu), _cu_dev(LENS_K, gpu), table.to(gpu)
    keep = (kpd.clone(), vpd.clone())
    cu_k = np.concatenate([[0], np.cumsum(LENS_K)])
    for msl_q, msl_k in ((128, P * ps), (MSL_Q, 100)):
        ref, owned = kv_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu_q, msl_q, cu_k, msl_k, causal)
        out = torch.full(q.shape, SENTINEL, dtype=dtype, device=gpu)
        ops.attention_varlen_paged(qd, kpd, vpd, cud, msl_q, td, su, max_seqlen_k=msl_k, causal=causal, out=out)
        o, own = out.cpu(), torch.from_numpy(owned.copy())
        assert int(owned.sum()) == sum(min(n, msl_q) for n in LENS_Q)
        assert (o[~own].float() == SENTINEL).all(), "a row of no sequence was written"
        assert (o[own].float() != SENTINEL).all(), "an owned row was not written"
        _gate(o[own], ref[owned], dtype, f"paged no-stray d={d} causal={causal} max_seqlen=({msl_q}, {msl_k})")
    assert _nan_eq(kpd, keep[0]) and _nan_eq(vpd, keep[1]), "the attention call wrote to the pool"


def _corrupt_cases():
    for e in CORRUPT_ENTRIES:
        yield f"entry {e}", e, None
    for name in sorted(CORRUPT_SEQUSED):
        yield f"seqused {name}", None, CORRUPT_SEQUSED[name]


CORRUPT_CASES = {name: (e, su) for name, e, su in _corrupt_cases()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORRUPT_CASES))
def test_varlen_paged_corrupt_arrays_are_clamped(gpu, name):
    """The replay's corrupt table entries and key counts, once each, on a pool that is finite
    everywhere: owned rows are finite, everything else keeps the sentinel, the guard blocks and rows
    around q, out and the pool are intact.  (That no access leaves the pool is the replay's result.)"""
    from exploring_flash_attention_amd import ops
    entry, su = CORRUPT_CASES[name]
    dtype, d, H, Hkv, ps, P = torch.bfloat16, 128, 4, 2, 64, 8
    nb, GB = len(LENS_Q) * P, 2
    g = torch.Generator().manual_seed(77)
    cu_q = np.concatenate([[0], np.cumsum(LENS_Q)])
    Tq = int(cu_q[-1])
    qb = torch.randn(Tq + 2 * GUARD, H, d, generator=g).to(dtype).to(gpu)
    kb, vb = (torch.randn(nb + 2 * GB, ps, Hkv, d, generator=g).to(dtype).to(gpu) for _ in range(2))
    table = np.random.default_rng(2).permutation(nb).astype(np.int64)
    if entry is not None:
        table[:] = nb if entry == "num_blocks" else entry
    keep = [t.clone() for t in (qb, kb, vb)]
    td = torch.tensor(table.tolist(), dtype=torch.int32, device=gpu).view(len(LENS_Q), P)
    lens_k = np.clip(LENS_K if su is None else su, 0, P * ps)
    for causal in (False, True):
        outb = torch.full((Tq + 2 * GUARD, H, d), SENTINEL, dtype=dtype, device=gpu)
        ops.attention_varlen_paged(qb[GUARD:GUARD + Tq], kb[GB:GB + nb], vb[GB:GB + nb], _cu_dev(cu_q, gpu), MSL_Q, td,
                                   _cu_dev(LENS_K if su is None else su, gpu), causal=causal, out=outb[GUARD:GUARD + Tq])
        torch.cuda.synchronize()
        o = outb.cpu().float()
        assert torch.isfinite(o).all()
        assert (o[:GUARD] == SENTINEL).all() and (o[GUARD + Tq:] == SENTINEL).all()
        assert (o[GUARD:GUARD + Tq] != SENTINEL).all(), (name, causal)
        # what the clamped arrays name, against fp64
        blocks = np.clip(table, 0, nb - 1).reshape(len(LENS_Q), P)
        kk, vv = (torch.cat([t[GB:GB + nb][blocks[b]].reshape(P * ps, Hkv, d)[:lens_k[b]] for b in range(len(LENS_Q))])
                  for t in (kb, vb))
        ref, owned = kv_ref(qb[GUARD:GUARD + Tq].cpu().double().numpy(), kk.cpu().double().numpy(),
                            vv.cpu().double().numpy(), cu_q, MSL_Q, np.concatenate([[0], np.cumsum(lens_k)]), P * ps, causal)
        assert owned.all()
        _gate(outb[GUARD:GUARD + Tq].cpu(), ref, dtype, f"paged corrupt {name} causal={causal}")
    assert all(torch.equal(a, b) for a, b in zip(keep, (qb, kb, vb)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_paged_chunked_prefill_end_to_end(gpu, d, dtype):
    """A causal sequence of 384 tokens (beside one of 200) in chunks: each chunk's K / V appended to
    a NaN-filled pool, then attended through the table.  128-token chunks reproduce the one-shot
    attention_varlen rows bit for bit; chunks of 100, 156 and 128 tokens pass the gate."""
    from exploring_flash_attention_amd import ops
    H, Hkv, LA, LB, ps, P = 4, 2, 384, 200, 64, 6
    q, k, v, cu, _ = _batch(d, H, Hkv, dtype, 8, (LA, LB))
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    ref, _ = varlen_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu, LA, True)
    one = ops.attention_varlen(qd, kd, vd, _cu_dev(cu, gpu), LA, causal=True)
    table = torch.tensor(np.random.default_rng(5).permutation(2 * P + 2)[:2 * P].tolist(), dtype=torch.int32,
                         device=gpu).view(2, P)
    for chunks, bitwise in (((128, 128, 128), True), ((100, 156, 128), False)):
        kp, vp = (torch.full((2 * P + 2, ps, Hkv, d), float("nan"), dtype=dtype, device=gpu) for _ in range(2))
        got = torch.empty_like(one[:LA])
        done = 0
        for n in chunks:
            qc = torch.cat([qd[done:done + n], qd[LA:LA + LB]])
            kc, vc = (torch.cat([t[done:done + n], t[LA:LA + LB]]) for t in (kd, vd))
            cuc, su = _cu_dev([0, n, n + LB], gpu), _cu_dev([done + n, LB], gpu)
            with ops.launched_kernels() as kl:
                ops.kv_cache_append_paged(kc, vc, kp, vp, cuc, max(n, LB), table, su)
                oc = ops.attention_varlen_paged(qc, kp, vp, cuc, max(n, LB), table, su, causal=True)
            assert kl[0] == f"fa_kv_append_kernel [grid {2 * -(-max(n, LB) // APPEND_ROWS) * Hkv}]", kl
            assert kl[1].startswith(_label(True, True)), kl
            got[done:done + n] = oc[:n]
            assert torch.equal(oc[n:], one[LA:LA + LB])      # the other sequence: s = 0 every time
            done += n
        if bitwise:
            assert torch.equal(got, one[:LA])
        _gate(got, ref[:LA], dtype, f"paged chunks {chunks} d={d}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (40, 128))
def test_kv_append_alone(gpu, d, dtype):
    """Old keys in the pool, a chunk appended: the pool gathered in table order is cat(old, new) bit
    for bit, every other element of the pool is untouched.  The new rows are the K / V slices of a
    fused QKV projection (strided, read in place); one chunk straddles a page boundary, one sequence
    has no new token, one starts an empty cache."""
    from exploring_flash_attention_amd import ops
    H, Hkv, ps, P = 4, 2, 64, 4
    old, new = (50, 64, 17, 0, 120), (30, 70, 0, 1, 8)      # 50..79 straddles; 64..133 starts a page; none; first; inside
    B, nb = len(old), len(old) * P + 2
    g = torch.Generator().manual_seed(9)
    cu = np.concatenate([[0], np.cumsum(new)])
    T = int(cu[-1]) + GUARD
    qkv = torch.randn(T, H + 2 * Hkv, d, generator=g).to(dtype).to(gpu)
    kn, vn = qkv[:, H:H + Hkv], qkv[:, H + Hkv:]
    assert not kn.is_contiguous() and kn.stride() == vn.stride()
    table = _table_for([P * ps] * B, ps, P, nb, seed=4)
    olds = [torch.randn(sum(old), Hkv, d, generator=g).to(dtype) for _ in range(2)]
    pools = [_scatter(o, old, ps, P, nb, table, torch.randn(nb, ps, Hkv, d, generator=g).to(dtype))[0].to(gpu)
             for o in olds]
    keep = [p.clone() for p in pools]
    td = torch.from_numpy(table).to(torch.int32).view(B, P).to(gpu)
    after = [o + n for o, n in zip(old, new)]
    with ops.launched_kernels() as kl:
        assert ops.kv_cache_append_paged(kn, vn, pools[0], pools[1], _cu_dev(cu, gpu), max(new), td, _cu_dev(after, gpu)) is None
    assert kl == [f"fa_kv_append_kernel [grid {B * -(-max(new) // APPEND_ROWS) * Hkv}]"], kl
    torch.cuda.synchronize()
    mask = torch.zeros(nb, ps, dtype=torch.bool)
    for b in range(B):
        for p in range(old[b], after[b]):
            mask[int(table[b * P + p // ps]), p % ps] = True
    assert int(mask.sum()) == sum(new)
    for pool, kept, o, nw in zip(pools, keep, olds, (kn, vn)):
        s = 0
        for b in range(B):
            seq = pool[td[b].long()].reshape(P * ps, Hkv, d)[:after[b]]
            want = torch.cat([o[s:s + old[b]].to(gpu), nw[int(cu[b]):int(cu[b + 1])]])
            assert torch.equal(seq, want), f"sequence {b}"
            s += old[b]
        # (bit patterns: the tails of the old keys' last pages hold NaN)
        assert _nan_eq(pool.cpu()[~mask], kept.cpu()[~mask]), "a row that no token owns was written"


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_paged_graph_replay_follows_the_arrays(gpu, causal):
    """One paged call captured on a side stream; block_table, seqused_k and cu_seqlens rewritten in
    place; every replay equals the eager result for the new arrays bit for bit."""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv, ps, P, nb = torch.bfloat16, 128, 4, 2, 64, 4, 16
    g = torch.Generator().manual_seed(41)
    q = torch.randn(171 + GUARD, H, d, generator=g).to(dtype).to(gpu)
    kp, vp = (torch.randn(nb, ps, Hkv, d, generator=g).to(dtype).to(gpu) for _ in range(2))
    rng = np.random.default_rng(6)
    rounds = [([0, 130, 170, 171], [200, 40, 7]), ([0, 100, 101, 171], [256, 0, 90]), ([0, 1, 131, 160], [64, 130, 1])]
    tables = [rng.permutation(nb)[:3 * P].reshape(3, P) for _ in rounds]
    dev = lambda a: torch.tensor(np.asarray(a).tolist(), dtype=torch.int32, device=gpu)   # noqa: E731
    wants = [ops.attention_varlen_paged(q, kp, vp, dev(cq), 130, dev(t), dev(s_), causal=causal,
                                        out=torch.full_like(q, SENTINEL)).clone()
             for (cq, s_), t in zip(rounds, tables)]
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[1], wants[2])
    cu, su, tbl = dev(rounds[0][0]), dev(rounds[0][1]), dev(tables[0])
    out = torch.empty_like(q)

    def call():
        return ops.attention_varlen_paged(q, kp, vp, cu, 130, tbl, su, causal=causal, out=out)

    s = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    for (cq, s_), t, want in zip(rounds, tables, wants):
        cu.copy_(dev(cq))
        su.copy_(dev(s_))
        tbl.copy_(dev(t))
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.gpu
def test_readout_varlen_paged(gpu):
    """Softmax-weight readout (tests/test_weight_readout_fwd.py's varlen probe and gate) through the
    paged key side: K, and the selector used as V, scattered into shuffled pages, len_k = len_q."""
    from exploring_flash_attention_amd import ops
    import test_weight_readout_fwd as W
    d, causal, H, Hkv, dtype, msl, ps = 128, True, 4, 2, torch.bfloat16, 257, 64
    q, k, cu, lens = W.varlen_inputs("steep", d, H, Hkv, dtype, msl, causal)
    lens_k = [min(n, msl) for n in lens]
    P = (max(lens_k) + ps - 1) // ps
    nb = len(lens) * P + 3
    table = _table_for(lens_k, ps, P, nb, seed=11)
    td = torch.from_numpy(table).to(torch.int32).view(len(lens), P).to(gpu)
    packed = lambda t: torch.cat([t[int(cu[b]):int(cu[b]) + n] for b, n in enumerate(lens_k)])   # noqa: E731
    kp = _scatter(packed(k), lens_k, ps, P, nb, table)[0].to(gpu)
    qd, cud, su = q.to(gpu), _cu_dev(cu, gpu), _cu_dev(lens_k, gpu)

    def call(v, out):
        vp = _scatter(packed(v), lens_k, ps, P, nb, table)[0].to(gpu)
        return ops.attention_varlen_paged(qd, kp, vp, cud, msl, td, su, causal=causal, out=out.to(gpu))

    with ops.launched_kernels() as kl:
        got = W.read_varlen(call, q, cu, lens, msl, Hkv, d, dtype)
    assert set(kl) == {f"{_label(causal, True)} [grid {len(lens) * H * 3}]"}, kl
    worst = W.gate_varlen(got, W.varlen_weights(q, k, cu, lens, msl, causal), dtype, "varlen paged")
    print(f"readout op=varlen_paged d={d} causal={causal} H={H}/{Hkv}: worst err/bound={worst:.3f}")
