"""Variable-length attention with key lengths of their own: fa_fwd_varlen_kv /
ops.attention_varlen(cu_seqlens_k=, max_seqlen_k=, seqused_k=) -- chunked prefill against a prefix.

q and o are [Tq, H, d] described by cu_seqlens, k and v [Tk, H_kv, d] described by cu_seqlens_k
(cut to the first seqused_k[b] rows where given).  Sequence b has len_q query and len_k key
tokens, s = len_k - len_q; a query row sees every key, or with `causal` position i sees keys
j <= i + s (bottom-right aligned).  A row that sees no key is zeros.

CPU part: the entry's argument checks (no launch), the Python-side checks, this file's fp64
reference against torch's scaled_dot_product_attention with an explicit mask, and a NumPy replay
of the KVLEN variant of csrc/fa_fwd_kernel.hpp for whole grids: item decode, the clamps of both
sides, kv_end, td0, the step schedule (which tiles are masked) and every descriptor.

GPU part: fp64 reference on the storage-rounded inputs under tests/test_varlen.py's GATE, and
bitwise comparisons against the self-attention call wherever both compute the same thing.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import exploring_flash_attention_amd._lib as L
from test_varlen import (CORRUPT, DTYPES, FAKE, GATE, GUARD, IDS, KBQ, NULL, SENTINEL, Alloc, _batch, _cu_dev, _gate,
                         bk_for, varlen_ref, xcd_remap)

INT32_MAX = 2 ** 31 - 1


def side_clamp(cu, T, max_seqlen):
    """The kernel's (start, len) of every sequence of one side: 64-bit, whatever cu holds."""
    cu = np.asarray(cu, np.int64)
    msl = min(int(max_seqlen), int(T))  # fa_capi.cpp
    st = np.clip(cu[:-1], 0, T)
    n = np.clip(cu[1:] - st, 0, np.minimum(T - st, msl))
    return st, n


def key_clamp(cu_k, Tk, max_seqlen_k, seqused=None):
    st, n = side_clamp(cu_k, Tk, max_seqlen_k) if Tk > 0 else (np.zeros(len(cu_k) - 1, np.int64),) * 2
    if seqused is not None:
        n = np.minimum(n, np.maximum(np.asarray(seqused, np.int64), 0))
    return st, n


def visible(len_q, len_k, causal):
    """[len_q, len_k] bool: the definition."""
    i, j = np.arange(len_q)[:, None], np.arange(len_k)[None, :]
    return (j <= i + (len_k - len_q)) if causal else np.ones((len_q, len_k), bool)


def kv_ref(q, k, v, cu_q, msl_q, cu_k, msl_k, causal, seqused=None):
    """fp64 reference on the clamped ranges (the identity on valid arrays).  Returns (o, owned): o
    [Tq, H, d] with NaN in the rows of no sequence and zeros in the rows that see no key."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    Tq, H, d = q.shape
    G = H // k.shape[1]
    stq, nq = side_clamp(cu_q, Tq, msl_q)
    stk, nk = key_clamp(cu_k, k.shape[0], msl_k, seqused)
    o = np.full((Tq, H, d), np.nan)
    owned = np.zeros(Tq, bool)
    for b in range(len(stq)):
        sq, lq, sk, lk = int(stq[b]), int(nq[b]), int(stk[b]), int(nk[b])
        if lq == 0:
            continue
        owned[sq:sq + lq] = True
        vis = visible(lq, lk, causal)
        some = vis.any(axis=1)
        for h in range(H):
            out = np.zeros((lq, d))
            if some.any():
                sc = np.where(vis[some], (q[sq:sq + lq, h][some] @ k[sk:sk + lk, h // G].T) / np.sqrt(d), -np.inf)
                p = np.exp(sc - sc.max(axis=-1, keepdims=True))
                out[some] = (p / p.sum(axis=-1, keepdims=True)) @ v[sk:sk + lk, h // G]
            o[sq:sq + lq, h] = out
    return o, owned


# ----------------------------------------------------------------------------------------
# CPU: the C entry's argument checks, the export, the Python-side checks, the reference
# ----------------------------------------------------------------------------------------


def _call(fn, q=FAKE, k=FAKE, v=FAKE, o=FAKE, cu=FAKE, cuk=FAKE, su=NULL, B=2, T=300, Tk=500, msl=200, mslk=400, H=4,
          Hkv=2, d=128, qs=None, kvs=None, os_=None, scale=0.1, flags=0, dtype=L.FA_DTYPE_BF16):
    return fn(q, k, v, o, cu, cuk, su, B, T, Tk, msl, mslk, H, Hkv, d, qs, kvs, os_, scale, flags, dtype, NULL)


def test_varlen_kv_entry_argument_checks():
    lib = L.lib()
    fn = lib.fa_fwd_varlen_kv
    err = lib.fa_last_error
    for name in ("q", "k", "v", "o"):
        assert _call(fn, **{name: NULL}) == L.FA_ERR_INVALID_ARG and b"null" in err()
    assert _call(fn, cu=NULL) == L.FA_ERR_INVALID_ARG and b"cu_seqlens" in err()
    assert _call(fn, cuk=NULL) == L.FA_ERR_INVALID_ARG and b"cu_seqlens_k" in err()
    assert _call(fn, cuk=ctypes.c_void_p(0x10002)) == L.FA_ERR_INVALID_ARG and b"cu_seqlens_k" in err()
    assert _call(fn, su=ctypes.c_void_p(0x10002)) == L.FA_ERR_INVALID_ARG and b"seqused_k" in err()
    for mslk in (0, -5):
        assert _call(fn, mslk=mslk) == L.FA_ERR_INVALID_ARG and b"max_seqlen_k" in err()
    for msl in (0, -5):
        assert _call(fn, msl=msl) == L.FA_ERR_INVALID_ARG and b"max_seqlen=" in err()
    assert _call(fn, Tk=-1) == L.FA_ERR_INVALID_ARG and b"total_tokens_k" in err()
    assert _call(fn, T=-1) == L.FA_ERR_INVALID_ARG and b"total_tokens=" in err()
    assert _call(fn, Tk=1 << 31) == L.FA_ERR_UNSUPPORTED and b"total_tokens_k" in err()
    assert _call(fn, T=1 << 31) == L.FA_ERR_UNSUPPORTED and b"total_tokens=" in err()
    for Hkv in (3, 0, 8, -1):
        assert _call(fn, Hkv=Hkv) == L.FA_ERR_INVALID_ARG and b"H_kv" in err()
    for flags in (2, 3, 0x80000000):
        assert _call(fn, flags=flags) == L.FA_ERR_INVALID_ARG and b"flags" in err()
    for d in (96, 384, 512):
        assert _call(fn, d=d) == L.FA_ERR_UNSUPPORTED and f"d={d}".encode() in err()
    assert _call(fn, dtype=L.FA_DTYPE_FP64) == L.FA_ERR_UNSUPPORTED and b"varlen" in err() and b"FP64" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(fn, scale=bad) == L.FA_ERR_INVALID_ARG and b"softmax_scale" in err()
    for B in (0, -1):
        assert _call(fn, B=B) == L.FA_ERR_INVALID_ARG and b"B=" in err()
    # the grid is the query side's
    assert _call(fn, B=1 << 20, H=1 << 10, Hkv=1 << 10, T=1 << 30, msl=1 << 10) == L.FA_ERR_UNSUPPORTED
    assert b"grid" in err()
    S2 = ctypes.c_int64 * 2
    for which in ("qs", "kvs", "os_"):
        for bad in ((1028, 128), (1024, 4), (0, 128), (1024, -8)):
            assert _call(fn, **{which: S2(*bad)}) == L.FA_ERR_INVALID_ARG and b"stride" in err()
        assert _call(fn, **{which: S2(64, 128)}) == L.FA_ERR_INVALID_ARG and b"token stride" in err()
        assert _call(fn, **{which: S2((1 << 20) + 8, 128)}) == L.FA_ERR_UNSUPPORTED and b"token stride" in err()
    # no query tokens: FA_OK, nothing launched (the pointers are fakes)
    assert _call(fn, T=0) == L.FA_OK and lib.fa_last_kernels() == b""


def test_varlen_kv_is_declared_and_exported():
    assert "fa_fwd_varlen_kv" in L.SIGNATURES and len(L.SIGNATURES["fa_fwd_varlen_kv"][1]) == 22
    assert len(L.SIGNATURES["fa_fwd_varlen"][1]) == 18  # the old entry keeps its signature
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fa_mi355x.h")) as f:
        text = f.read()
    assert "int fa_fwd_varlen_kv(" in text and "int fa_fwd_varlen(" in text
    assert hasattr(L.lib(), "fa_fwd_varlen_kv")


def test_varlen_kv_python_side_checks():
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q, kv, kv2 = torch.zeros(10, 4, 64, dtype=bf), torch.zeros(10, 2, 64, dtype=bf), torch.zeros(30, 2, 64, dtype=bf)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    cuk = torch.tensor([0, 20, 30], dtype=torch.int32)
    su = torch.tensor([5, 5], dtype=torch.int32)
    av = ops.attention_varlen
    with pytest.raises(ValueError, match="max_seqlen_k"):
        av(q, kv2, kv2, cu, 6, cu_seqlens_k=cuk)
    with pytest.raises(ValueError, match="seqused_k is only valid together with cu_seqlens_k"):
        av(q, kv, kv, cu, 6, seqused_k=su)
    with pytest.raises(ValueError, match="max_seqlen_k is only valid together with cu_seqlens_k"):
        av(q, kv, kv, cu, 6, max_seqlen_k=20)
    with pytest.raises(ValueError, match="disagree"):  # Tq != Tk without cu_seqlens_k
        av(q, kv2, kv2, cu, 6)
    with pytest.raises(TypeError, match="cu_seqlens_k"):
        av(q, kv2, kv2, cu, 6, cu_seqlens_k=[0, 20, 30], max_seqlen_k=20)
    with pytest.raises(TypeError, match="seqused_k"):
        av(q, kv2, kv2, cu, 6, cu_seqlens_k=cuk, max_seqlen_k=20, seqused_k=[5, 5])
    for bad in (cuk.long(), cuk.reshape(1, 3), cuk[:2], torch.zeros(4, dtype=torch.int32)):  # dtype, shape
        with pytest.raises(ValueError, match="cu_seqlens_k must be an int32"):
            av(q, kv2, kv2, cu, 6, cu_seqlens_k=bad, max_seqlen_k=20)
    for bad in (su.long(), su.reshape(1, 2), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="seqused_k must be an int32"):
            av(q, kv2, kv2, cu, 6, cu_seqlens_k=cuk, max_seqlen_k=20, seqused_k=bad)
    with pytest.raises(ValueError, match="max_seqlen_k=-1"):
        av(q, kv2, kv2, cu, 6, cu_seqlens_k=cuk, max_seqlen_k=-1)
    with pytest.raises(TypeError):  # keyword-only
        av(q, kv2, kv2, cu, 6, False, None, cuk, 20)
    with pytest.raises(ValueError, match="no CPU fallback"):  # device: everything on the host
        av(q, kv2, kv2, cu, 6, cu_seqlens_k=cuk, max_seqlen_k=20, seqused_k=su)


def test_kv_reference_matches_torch_sdpa():
    g = torch.Generator().manual_seed(12)
    pairs = ((5, 9), (7, 7), (1, 30), (9, 4), (12, 1), (0, 6), (6, 0), (20, 33))
    cu_q = np.concatenate([[0], np.cumsum([p[0] for p in pairs])])
    cu_k = np.concatenate([[0], np.cumsum([p[1] for p in pairs])])
    H, Hkv, d = 4, 2, 16
    q = torch.randn(int(cu_q[-1]) + 3, H, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(int(cu_k[-1]) + 2, Hkv, d, generator=g, dtype=torch.float64) for _ in range(2))
    for causal in (False, True):
        got, owned = kv_ref(q.numpy(), k.numpy(), v.numpy(), cu_q, 64, cu_k, 64, causal)
        assert owned.sum() == cu_q[-1] and not owned[int(cu_q[-1]):].any() and np.isnan(got[~owned]).all()
        for b, (lq, lk) in enumerate(pairs):
            if lq == 0:
                continue
            sq, sk = int(cu_q[b]), int(cu_k[b])
            vis = visible(lq, lk, causal)
            some = vis.any(axis=1)
            assert (got[sq:sq + lq][~some] == 0).all()   # rows that see no key: zeros
            if not some.any():
                continue
            qs = q[sq:sq + lq].transpose(0, 1)
            ks, vs = (t[sk:sk + lk].transpose(0, 1).repeat_interleave(H // Hkv, dim=0) for t in (k, v))
            want = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=torch.from_numpy(vis))
            diff = np.abs(got[sq:sq + lq] - want.transpose(0, 1).numpy())[some]
            assert diff.max() <= 1e-12, (b, causal, diff.max())
    # equal lengths: the self-attention reference of tests/test_varlen.py
    for causal in (False, True):
        a, _ = kv_ref(q.numpy()[:40], k.numpy()[:40], v.numpy()[:40], [0, 13, 40], 64, [0, 13, 40], 64, causal)
        b, _ = varlen_ref(q.numpy()[:40], k.numpy()[:40], v.numpy()[:40], [0, 13, 40], 64, causal)
        assert np.abs(a - b).max() <= 1e-12
    # seqused_k cuts the range to its first rows; negative counts as 0, huge as the range
    a, _ = kv_ref(q.numpy(), k.numpy(), v.numpy(), cu_q[:3], 64, [0, 9, 16], 64, True, seqused=[4, INT32_MAX])
    b, _ = kv_ref(q.numpy(), k.numpy(), v.numpy(), cu_q[:3], 64, [0, 4, 4], 64, True)
    assert np.array_equal(a[:5], b[:5])
    c, _ = kv_ref(q.numpy(), k.numpy(), v.numpy(), cu_q[:3], 64, [0, 9, 16], 64, True)
    assert np.array_equal(a[5:12], c[5:12])
    z, _ = kv_ref(q.numpy(), k.numpy(), v.numpy(), cu_q[:3], 64, [0, 9, 16], 64, False, seqused=[-3, 2])
    assert (z[:5] == 0).all()


# ----------------------------------------------------------------------------------------
# CPU: replay of the KVLEN variant (csrc/fa_fwd_kernel.hpp) -- schedule, masks, addresses
# ----------------------------------------------------------------------------------------


def item_schedule(qt, len_q, len_k, bk, causal):
    """One work item's key range and step schedule, as the kernel computes them.  Returns (nkv,
    ntiles, td0, masked): masked[t] says whether tile t goes through cmask (causal) -- the steps
    are replayed flag by flag, and every tile must be the subject of exactly one step."""
    s = len_k - len_q
    if not causal:
        nkv = len_k
        return nkv, (nkv + bk - 1) // bk, 0, None
    nkv = min(max(s + KBQ * (qt + 1), 0), len_k)
    ntiles = (nkv + bk - 1) // bk
    td0 = (max(s + KBQ * qt, 0) // bk) & ~1
    if nkv <= 0:
        return nkv, 0, td0, []
    masked = [False] * ntiles
    steps = []

    def run(t, more, cmnext):
        steps.append(t)
        assert t < ntiles and (not more or t + 1 < ntiles), "a step past the last tile"
        if more and cmnext:
            masked[t + 1] = True

    if td0 == 0:
        masked[0] = True                       # the prologue
    t = 0
    while t + 2 < td0:
        run(t, True, False), run(t + 1, True, False)
        t += 2
    if td0 > 0:
        run(t, True, False), run(t + 1, True, True)
        t += 2
    while t + 2 < ntiles:
        run(t, True, True), run(t + 1, True, True)
        t += 2
    if ntiles - t == 2:
        run(t, True, True), run(t + 1, False, False)
    else:
        run(t, False, False)
    assert steps == list(range(ntiles)), (steps, ntiles)
    return nkv, ntiles, td0, masked


def unmasked_pairs(len_q, len_k, bk, causal):
    """[len_q, len_k'] bool of the (row, key) pairs the kernel leaves unmasked, over all query
    tiles; keys past len_k that an unmasked tile would let through make the array wider."""
    width = len_k + 2 * bk + KBQ
    seen = np.zeros((len_q, width), bool)
    rows_done = np.zeros(len_q, bool)
    for qt in range((len_q + KBQ - 1) // KBQ):
        r0, r1 = qt * KBQ, min(qt * KBQ + KBQ, len_q)
        rows_done[r0:r1] = True
        nkv, ntiles, td0, masked = item_schedule(qt, len_q, len_k, bk, causal)
        if nkv <= 0:
            continue                           # the zero-store exit
        rows = np.arange(r0, r1)
        for t in range(ntiles):
            keys = np.arange(t * bk, (t + 1) * bk)
            if causal and masked[t]:
                last = np.clip(rows + (len_k - len_q), -1, nkv - 1)     # cmask
                seen[r0:r1, keys] |= keys[None, :] <= last[:, None]
            elif causal:
                seen[r0:r1, keys] = True                                # a steady, unmasked tile
            else:
                seen[r0:r1, keys] |= (keys < nkv)[None, :]              # mask(): the key tail
    assert rows_done.all()
    return seen


@pytest.mark.parametrize("bk", (64, 32))
@pytest.mark.parametrize("len_q", (1, 64, 129))
def test_replay_unmasked_pairs_equal_the_definition(len_q, bk):
    for s in range(-130, 131):
        len_k = len_q + s
        if len_k < 0:
            continue
        for causal in (True, False):
            got = unmasked_pairs(len_q, len_k, bk, causal)
            want = np.zeros_like(got)
            want[:, :len_k] = visible(len_q, len_k, causal)
            assert np.array_equal(got, want), (len_q, len_k, bk, causal)


def test_replay_td0_parity_and_long_prefixes():
    """Diagonals deep inside a long prefix: td0 odd before rounding, several unmasked pairs."""
    for bk in (64, 32):
        for len_q, len_k in ((129, 1000), (257, 321), (64, 128), (128, 129), (300, 300 + 7 * bk), (5, 5 + 3 * bk)):
            got = unmasked_pairs(len_q, len_k, bk, True)
            assert np.array_equal(got[:, :len_k], visible(len_q, len_k, True)) and not got[:, len_k:].any()
            for qt in range((len_q + KBQ - 1) // KBQ):
                nkv, ntiles, td0, masked = item_schedule(qt, len_q, len_k, bk, True)
                assert td0 % 2 == 0 and td0 < ntiles and not any(masked[:td0]) and all(masked[td0:])


def replay_kv(cu_q, cu_k, seqused, Tq, Tk, msl_q, msl_k, H, Hkv, D, causal, strides, allocs, valid=True,
              clamp_k=True):
    """Replay one fa_fwd_varlen_kv launch.  strides: ({token, head} of q, of k/v, of o).  Asserts:
    the decode is a bijection; every Q descriptor lies in q and in the own query range; every K/V
    descriptor lies in k / v and in the own key range; the stored rows are disjoint and exactly the
    rows below len_q.  Returns (running items, zero-store items, stored rows)."""
    cu_q, cu_k = np.asarray(cu_q, np.int64), np.asarray(cu_k, np.int64)
    B = len(cu_q) - 1
    assert len(cu_k) == B + 1
    nqt = (min(msl_q, Tq) + KBQ - 1) // KBQ
    G = H // Hkv
    nblk = B * H * nqt
    assert 0 < nblk < 1 << 31
    blk = np.arange(nblk, dtype=np.int64)
    w = xcd_remap(blk, nblk)
    if causal:
        g, rest = w % G, w // G
        qt, bh = nqt - 1 - rest % nqt, (rest // nqt) * G + g
    else:
        qt, bh = w % nqt, w // nqt
    b, h = bh // H, bh % H
    assert np.array_equal(np.sort((b * H + h) * nqt + qt), blk), "decode is not a bijection"
    stq, nq = side_clamp(cu_q, Tq, msl_q)
    if clamp_k:
        stk, nk = key_clamp(cu_k, Tk, msl_k, seqused)
    else:  # the planted defect: no clamp of the key side against Tk
        stk, nk = cu_k[:-1], np.minimum(cu_k[1:] - cu_k[:-1], msl_k)
    assert ((stq + nq <= Tq) & (stq >= 0) & (nq >= 0)).all()
    assert not clamp_k or ((stk + nk <= Tk) & (stk >= 0) & (nk >= 0)).all()
    (qs, ks, os_), ROWB, bk = strides, 2 * D, bk_for(D)
    qrb, krb = 2 * qs[0], 2 * ks[0]
    stored, items, zero_items = [], 0, 0
    for i in np.nonzero(qt * KBQ < nq[b])[0]:     # the others return before any barrier or DMA
        bi, hi, qti = int(b[i]), int(h[i]), int(qt[i])
        sq, lq, sk, lk = int(stq[bi]), int(nq[bi]), int(stk[bi]), int(nk[bi])
        if valid:
            assert int(cu_q[bi]) <= sq and sq + lq <= int(cu_q[bi + 1])
            assert int(cu_k[bi]) <= sk and sk + lk <= int(cu_k[bi + 1])
        q_tile0 = qti * KBQ
        q_rows = min(lq - q_tile0, KBQ)
        nkv, ntiles, td0, masked = item_schedule(qti, lq, lk, bk, causal)
        for r in range(q_tile0, q_tile0 + q_rows):   # O rows: the zero store and the epilogue alike
            allocs["o"].check(2 * ((sq + r) * os_[0] + hi * os_[1]), ROWB, "O row")
            stored.append((bi, hi, r, sq + r))
        if nkv <= 0:
            zero_items += 1
            continue
        items += 1
        q_base = 2 * (sq * qs[0] + hi * qs[1]) + q_tile0 * qrb
        q_len = (q_rows - 1) * qrb + ROWB
        allocs["q"].check(q_base, q_len, "Q descriptor")
        first = (q_base - 2 * hi * qs[1]) // qrb
        last = (q_base + q_len - ROWB - 2 * hi * qs[1]) // qrb
        assert sq <= first and last < sq + lq, "Q descriptor leaves its sequence"
        assert 0 < nkv <= lk and td0 < ntiles
        k_head = 2 * (sk * ks[0] + (hi // G) * ks[1])
        for t in range(ntiles + 2):                  # (two prefetches past the end: empty descriptors)
            vld = min(max(nkv - t * bk, 0), bk)
            if t >= ntiles:
                assert vld == 0
                continue
            base, length = k_head + t * bk * krb, (vld - 1) * krb + ROWB
            for name in ("k", "v"):
                allocs[name].check(base, length, f"{name.upper()} tile {t}")
            kfirst = (base - 2 * (hi // G) * ks[1]) // krb
            klast = (base + length - ROWB - 2 * (hi // G) * ks[1]) // krb
            assert sk <= kfirst and klast < sk + lk, "K/V descriptor leaves its key range"
    per_seq = {(bi, hi, r) for bi, hi, r, _ in stored}
    assert len(per_seq) == len(stored), "two items store the same row"
    want = {(bi, hi, r) for bi in range(B) for hi in range(H) for r in range(int(nq[bi]))}
    assert per_seq == want, "stored rows are not exactly the rows below each query length"
    if valid:
        tok = {(row, hi) for _, hi, _, row in stored}
        assert len(tok) == len(stored), "two sequences store the same token row"
    return items, zero_items, stored


def _contig_kv(Tq, Tk, H, Hkv, D):
    strides = ((H * D, D), (Hkv * D, D), (H * D, D))
    allocs = {"q": Alloc("q", 2 * Tq * H * D), "k": Alloc("k", 2 * Tk * Hkv * D), "v": Alloc("v", 2 * Tk * Hkv * D),
              "o": Alloc("o", 2 * Tq * H * D)}
    return strides, allocs


# (len_q, len_k): a single row against a single key; a decode-like row; s = 0; s = kBK, td0 odd;
# s = 1; s = 63; a second query tile of one row and a long prefix; three query tiles, s = 64;
# s < 0, rows 0-29 zero; s < 0 across a tile boundary, tile 1 straddles; no queries; no keys
PAIRS = ((1, 1), (1, 200), (70, 70), (64, 128), (128, 129), (100, 163), (129, 300), (257, 321), (50, 20), (130, 2),
         (0, 40), (40, 0))
PAIRS_256 = PAIRS + ((96, 128), (33, 64))  # s = 32 = kBK at d = 256
MSL_Q, MSL_K = 257, 321


def _pairs(d):
    return PAIRS_256 if d == 256 else PAIRS


def _cus(pairs):
    return (np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).astype(np.int64),
            np.concatenate([[0], np.cumsum([p[1] for p in pairs])]).astype(np.int64))


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("D", (32, 64, 128, 256))
@pytest.mark.parametrize("H,Hkv", ((4, 4), (4, 2), (4, 1)))
def test_replay_kv_ragged_batch(H, Hkv, D, causal):
    pairs = _pairs(D)
    cu_q, cu_k = _cus(pairs)
    Tq, Tk = int(cu_q[-1]) + GUARD, int(cu_k[-1]) + GUARD
    items, zeros, stored = replay_kv(cu_q, cu_k, None, Tq, Tk, MSL_Q, MSL_K, H, Hkv, D, causal,
                                     *_contig_kv(Tq, Tk, H, Hkv, D))
    assert len(stored) == H * sum(p[0] for p in pairs)
    assert items + zeros == H * sum((p[0] + KBQ - 1) // KBQ for p in pairs)
    # (40, 0) always; causal: (130, 2)'s first tile lies above the diagonal (s + 128 <= 0)
    assert zeros == H * (2 if causal else 1)


CORRUPT_SEQUSED = {"negative": [-5, -2 ** 31, 3, 0, -1], "huge": [INT32_MAX, 10 ** 9, 5000, 451, INT32_MAX],
                   "mixed": [-1, INT32_MAX, 0, 1, 449]}
CORRUPT_LENS_Q = (130, 1, 64, 50, 129)


def _corrupt_cases():
    for name in sorted(CORRUPT):
        yield f"cu_k {name}", CORRUPT[name], None
    for name in sorted(CORRUPT_SEQUSED):
        yield f"seqused {name}", [0, 100, 200, 300, 400, 450], CORRUPT_SEQUSED[name]
    yield "both", CORRUPT["beyond T"], CORRUPT_SEQUSED["huge"]


CORRUPT_CASES = {name: (cu_k, su) for name, cu_k, su in _corrupt_cases()}


def _corrupt_q(cu_k):
    B = len(cu_k) - 1
    return np.concatenate([[0], np.cumsum(CORRUPT_LENS_Q[:B])]).astype(np.int64)


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("name", sorted(CORRUPT_CASES))
def test_replay_kv_corrupt_key_arrays_stay_inside(name, causal):
    """Whatever cu_seqlens_k and seqused_k hold, every descriptor stays inside rows [0, Tk): no
    guard rows in the allocations here."""
    cu_k, su = CORRUPT_CASES[name]
    su = None if su is None else su[:len(cu_k) - 1]
    cu_q = _corrupt_q(cu_k)
    Tq, Tk = int(cu_q[-1]), 450
    for msl_k in (257, 10000):
        replay_kv(cu_q, cu_k, su, Tq, Tk, 130, msl_k, 4, 2, 128, causal, *_contig_kv(Tq, Tk, 4, 2, 128), valid=False)
    # a corrupt query side with a valid key side, too
    for qname in sorted(CORRUPT):
        cq = CORRUPT[qname]
        ck = np.arange(len(cq)) * 90
        replay_kv(cq, ck, None, 450, 450, 10000, 90, 4, 2, 128, causal, *_contig_kv(450, 450, 4, 2, 128), valid=False)


def test_replay_kv_catches_a_missing_key_clamp():
    cu_k = CORRUPT["beyond T"]
    cu_q = _corrupt_q(cu_k)
    Tq = int(cu_q[-1])
    with pytest.raises(AssertionError, match="leaves"):
        replay_kv(cu_q, cu_k, None, Tq, 450, 130, 10000, 4, 2, 128, False, *_contig_kv(Tq, 450, 4, 2, 128),
                  valid=False, clamp_k=False)


CACHE_LMAX, CACHE_LENS, CACHE_LENS_Q = 256, (200, 1, 256, 0), (70, 1, 130, 5)


@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("D", (128, 256))
def test_replay_kv_padded_cache_view(D, causal):
    """A [B, Lmax, H_kv, d] cache viewed as [B * Lmax, H_kv, d]: K/V descriptors stay inside the
    first seqused_k[b] rows of slot b (asserted against the clamped range by replay_kv)."""
    B = len(CACHE_LENS)
    cu_q = np.concatenate([[0], np.cumsum(CACHE_LENS_Q)])
    cu_k = np.arange(B + 1) * CACHE_LMAX
    Tq, Tk = int(cu_q[-1]), B * CACHE_LMAX
    items, zeros, _ = replay_kv(cu_q, cu_k, CACHE_LENS, Tq, Tk, 130, CACHE_LMAX, 8, 2, D, causal,
                                *_contig_kv(Tq, Tk, 8, 2, D))
    assert zeros == 8 and items == 8 * 4
    stk, nk = key_clamp(cu_k, Tk, CACHE_LMAX, CACHE_LENS)
    assert nk.tolist() == list(CACHE_LENS) and stk.tolist() == [0, 256, 512, 768]


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _kv_batch(d, H, Hkv, dtype, seed=0, pairs=None):
    """Seeded packed inputs (host, storage-rounded) with GUARD rows past both cu[-1]."""
    pairs = _pairs(d) if pairs is None else pairs
    cu_q, cu_k = _cus(pairs)
    g = torch.Generator().manual_seed(100 + seed)
    q = torch.randn(int(cu_q[-1]) + GUARD, H, d, generator=g).to(dtype)
    k, v = (torch.randn(int(cu_k[-1]) + GUARD, Hkv, d, generator=g).to(dtype) for _ in range(2))
    return q, k, v, cu_q, cu_k


@functools.lru_cache(maxsize=None)
def _kv_ref(d, H, Hkv, dtype, causal, msl_q=MSL_Q, msl_k=MSL_K, seed=0, pairs=None):
    q, k, v, cu_q, cu_k = _kv_batch(d, H, Hkv, dtype, seed, pairs)
    o, owned = kv_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu_q, msl_q, cu_k, msl_k, causal)
    o.setflags(write=False)
    owned.setflags(write=False)
    return o, owned


def _label(causal, gqa):
    return "fa_fwd_kernel<final, varlen, kv" + (", causal" if causal else "") + (", gqa" if gqa else "") + ">"


def _sentinel(shape, dtype, gpu):
    return torch.full(tuple(shape), SENTINEL, dtype=dtype, device=gpu)


def _no_key_rows(ref, owned):
    """Owned rows whose reference is exactly zero in every head and column: they see no key."""
    return owned & (ref == 0).all(axis=(1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (32, 64, 128, 256))
@pytest.mark.parametrize("H,Hkv", ((4, 4), (4, 2), (4, 1)), ids=("mha", "gqa2", "mqa"))
def test_varlen_kv_matches_fp64_reference(gpu, H, Hkv, d, causal, dtype):
    """One ragged batch holding every edge at once (PAIRS)."""
    from exploring_flash_attention_amd import ops
    q, k, v, cu_q, cu_k = _kv_batch(d, H, Hkv, dtype)
    ref, owned = _kv_ref(d, H, Hkv, dtype, causal)
    out = _sentinel(q.shape, dtype, gpu)
    with ops.launched_kernels() as kl:
        o = ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu_q, gpu), MSL_Q, causal=causal, out=out,
                                 cu_seqlens_k=_cu_dev(cu_k, gpu), max_seqlen_k=MSL_K)
    assert o is out
    assert kl == [f"{_label(causal, Hkv < H)} [grid {len(_pairs(d)) * H * 3}]"], kl
    o = o.cpu()
    own = torch.from_numpy(owned.copy())
    assert torch.isfinite(o.float()).all()
    assert (o[~own].float() == SENTINEL).all(), "a row of no sequence was written"
    nokey = _no_key_rows(ref, owned)
    want_nokey = 40 + (30 + 128 if causal else 0)   # (40, 0); causal: (50, 20) rows 0-29, (130, 2) rows 0-127
    assert int(nokey.sum()) == want_nokey
    assert (o[torch.from_numpy(nokey)].float() == 0).all(), "a row that sees no key is not exactly zero"
    _gate(o[own], ref[owned], dtype, f"varlen kv H{H}/{Hkv} d={d} causal={causal} {IDS[dtype]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128))
def test_varlen_kv_no_stray_stores(gpu, d, causal, dtype):
    """out preset to a sentinel: with max_seqlen = 128 the query positions >= 128 and the guard rows
    keep it; with max_seqlen_k = 100 the longer key ranges are truncated to their first 100 rows."""
    from exploring_flash_attention_amd import ops
    H, Hkv = 4, 2
    q, k, v, cu_q, cu_k = _kv_batch(d, H, Hkv, dtype)
    qd, kd, vd, cqd, ckd = q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu_q, gpu), _cu_dev(cu_k, gpu)
    for msl_q, msl_k in ((MSL_Q, MSL_K), (128, MSL_K), (MSL_Q, 100)):
        ref, owned = _kv_ref(d, H, Hkv, dtype, causal, msl_q, msl_k)
        assert owned.sum() == sum(min(p[0], msl_q) for p in PAIRS) and not owned[-GUARD:].any()
        out = _sentinel(q.shape, dtype, gpu)
        ops.attention_varlen(qd, kd, vd, cqd, msl_q, causal=causal, out=out, cu_seqlens_k=ckd, max_seqlen_k=msl_k)
        o = out.cpu()
        own = torch.from_numpy(owned.copy())
        assert (o[~own].float() == SENTINEL).all(), f"a row of no sequence was written ({msl_q}, {msl_k})"
        assert (o[own].float() != SENTINEL).all(), f"an owned row was not written ({msl_q}, {msl_k})"
        _gate(o[own], ref[owned], dtype, f"kv no-stray d={d} causal={causal} max_seqlen=({msl_q}, {msl_k})")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128))
def test_varlen_kv_same_lengths_is_bitwise_the_self_attention_call(gpu, d, causal, dtype):
    """cu_seqlens_k = cu_seqlens on the same tokens (tests/test_varlen.py's ragged batch)."""
    from exploring_flash_attention_amd import ops
    H, Hkv = 4, 2
    q, k, v, cu, lens = _batch(d, H, Hkv, dtype)
    qd, kd, vd, cud = q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu, gpu)
    want, got = _sentinel(q.shape, dtype, gpu), _sentinel(q.shape, dtype, gpu)
    with ops.launched_kernels() as kl:
        ops.attention_varlen(qd, kd, vd, cud, 257, causal=causal, out=want)
        ops.attention_varlen(qd, kd, vd, cud, 257, causal=causal, out=got, cu_seqlens_k=cud.clone(), max_seqlen_k=257)
    assert ", kv" not in kl[0] and kl[1].startswith(_label(causal, True)), kl
    assert torch.equal(got, want)
    assert (got[:int(cu[-1])].float() != SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128, 256))
def test_varlen_kv_chunked_prefill(gpu, d, dtype):
    """A causal sequence of 384 tokens (beside one of 200) as chunks against the growing prefix:
    128-token chunks reproduce the one-shot call's rows bit for bit (the same tiles in the same
    order); chunks of 100, 156 and 128 tokens cut the tiles elsewhere and pass the gate."""
    from exploring_flash_attention_amd import ops
    H, Hkv, LA, LB = 4, 2, 384, 200
    q, k, v, cu, _ = _batch(d, H, Hkv, dtype, 8, (LA, LB))
    qd, kd, vd = q.to(gpu), k.to(gpu), v.to(gpu)
    ref, _ = varlen_ref(q.double().numpy(), k.double().numpy(), v.double().numpy(), cu, LA, True)
    one = ops.attention_varlen(qd, kd, vd, _cu_dev(cu, gpu), LA, causal=True)
    _gate(one[:LA + LB], ref[:LA + LB], dtype, f"one-shot d={d}")
    for chunks, bitwise in (((128, 128, 128), True), ((100, 156, 128), False)):
        got = torch.empty_like(one[:LA])
        done = 0
        for n in chunks:
            qc = torch.cat([qd[done:done + n], qd[LA:LA + LB]])
            kc, vc = (torch.cat([t[:done + n], t[LA:LA + LB]]) for t in (kd, vd))
            with ops.launched_kernels() as kl:
                oc = ops.attention_varlen(qc, kc, vc, _cu_dev([0, n, n + LB], gpu), max(n, LB), causal=True,
                                          cu_seqlens_k=_cu_dev([0, done + n, done + n + LB], gpu),
                                          max_seqlen_k=done + n + LB)
            assert kl[0].startswith(_label(True, True)), kl
            got[done:done + n] = oc[:n]
            assert torch.equal(oc[n:], one[LA:LA + LB])  # the other sequence: s = 0 every time
            done += n
        if bitwise:
            assert torch.equal(got, one[:LA])
        _gate(got, ref[:LA], dtype, f"chunks {chunks} d={d}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("d", (64, 128, 256))
def test_varlen_kv_seqused_on_a_padded_cache(gpu, d, causal):
    """A [B, 256, H_kv, d] cache read in place through seqused_k: bitwise the call on the same keys
    packed contiguously; the NaN past each length never reaches the output."""
    from exploring_flash_attention_amd import ops
    dtype, H, Hkv, B, Lmax = torch.bfloat16, 4, 2, len(CACHE_LENS), CACHE_LMAX
    g = torch.Generator().manual_seed(21)
    cu_q = np.concatenate([[0], np.cumsum(CACHE_LENS_Q)])
    q = torch.randn(int(cu_q[-1]), H, d, generator=g).to(dtype).to(gpu)
    kc, vc = (torch.randn(B, Lmax, Hkv, d, generator=g).to(dtype) for _ in range(2))
    packed_k = torch.cat([kc[b, :n] for b, n in enumerate(CACHE_LENS)]).to(gpu)
    packed_v = torch.cat([vc[b, :n] for b, n in enumerate(CACHE_LENS)]).to(gpu)
    for b, n in enumerate(CACHE_LENS):
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    kc, vc = kc.to(gpu), vc.to(gpu)
    cqd = _cu_dev(cu_q, gpu)
    want = ops.attention_varlen(q, packed_k, packed_v, cqd, 130, causal=causal,
                                cu_seqlens_k=_cu_dev(np.concatenate([[0], np.cumsum(CACHE_LENS)]), gpu),
                                max_seqlen_k=Lmax)
    got = ops.attention_varlen(q, kc.view(B * Lmax, Hkv, d), vc.view(B * Lmax, Hkv, d), cqd, 130, causal=causal,
                               cu_seqlens_k=_cu_dev(np.arange(B + 1) * Lmax, gpu), max_seqlen_k=Lmax,
                               seqused_k=_cu_dev(CACHE_LENS, gpu))
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    ref, owned = kv_ref(q.cpu().double().numpy(), packed_k.cpu().double().numpy(), packed_v.cpu().double().numpy(),
                        cu_q, 130, np.concatenate([[0], np.cumsum(CACHE_LENS)]), Lmax, causal)
    assert owned.all() and (got[-5:] == 0).all()      # the sequence without keys
    _gate(got, ref, dtype, f"padded cache d={d} causal={causal}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORRUPT_CASES))
def test_varlen_kv_corrupt_key_arrays_are_clamped(gpu, name):
    """Each corrupt cu_seqlens_k / seqused_k of the replay test, once: the rows the clamped query
    side names are finite, everything else keeps the sentinel, and the guard rows around q, k, v
    and out are intact.  (That no access can leave the tensors is what the CPU replay shows.)"""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv, Tk = torch.bfloat16, 128, 4, 2, 450
    cu_k, su = CORRUPT_CASES[name]
    su = None if su is None else su[:len(cu_k) - 1]
    cu_q = _corrupt_q(cu_k)
    Tq = int(cu_q[-1])
    g = torch.Generator().manual_seed(6)
    qb = torch.randn(Tq + 2 * GUARD, H, d, generator=g).to(dtype).to(gpu)
    kb, vb = (torch.randn(Tk + 2 * GUARD, Hkv, d, generator=g).to(dtype).to(gpu) for _ in range(2))
    keep = [t.clone() for t in (qb, kb, vb)]
    for causal, msl_k in ((False, 257), (True, 10000)):
        outb = _sentinel((Tq + 2 * GUARD, H, d), dtype, gpu)
        ops.attention_varlen(qb[GUARD:GUARD + Tq], kb[GUARD:GUARD + Tk], vb[GUARD:GUARD + Tk], _cu_dev(cu_q, gpu), 130,
                             causal=causal, out=outb[GUARD:GUARD + Tq], cu_seqlens_k=_cu_dev(cu_k, gpu),
                             max_seqlen_k=msl_k, seqused_k=None if su is None else _cu_dev(su, gpu))
        torch.cuda.synchronize()
        o = outb.cpu().float()
        assert torch.isfinite(o).all()
        assert (o[:GUARD] == SENTINEL).all() and (o[GUARD + Tq:] == SENTINEL).all()
        assert (o[GUARD:GUARD + Tq] != SENTINEL).all(), (name, causal)   # every query row exists here
        ref, owned = kv_ref(qb[GUARD:GUARD + Tq].cpu().double().numpy(), kb[GUARD:GUARD + Tk].cpu().double().numpy(),
                            vb[GUARD:GUARD + Tk].cpu().double().numpy(), cu_q, 130, cu_k, msl_k, causal, su)
        _gate(outb[GUARD:GUARD + Tq].cpu(), ref, dtype, f"corrupt {name} causal={causal}")
    assert all(torch.equal(a, b) for a, b in zip(keep, (qb, kb, vb)))


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_kv_reads_strided_tensors_in_place(gpu, causal, monkeypatch):
    """q as a slice of a fused [Tq, (H + 2 H_kv) d] projection, k and v as slices of a cache whose
    rows hold both ([Tk, 2, H_kv, 2 d]: strided tokens and heads), out a strided view: the views' own
    pointers and strides reach the library, no device memory is allocated, bitwise the contiguous
    call's result."""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv = torch.bfloat16, 128, 4, 2
    q, k, v, cu_q, cu_k = _kv_batch(d, H, Hkv, dtype, 5)
    Tq, Tk = q.shape[0], k.shape[0]
    cqd, ckd = _cu_dev(cu_q, gpu), _cu_dev(cu_k, gpu)
    want = _sentinel(q.shape, dtype, gpu)
    ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), cqd, MSL_Q, causal=causal, out=want, cu_seqlens_k=ckd,
                         max_seqlen_k=MSL_K)
    qkv = torch.zeros(Tq, H + 2 * Hkv, d, dtype=dtype)
    qkv[:, :H] = q
    qv = qkv.to(gpu)[:, :H]
    cache = torch.zeros(Tk, 2, Hkv, 2 * d, dtype=dtype)
    cache[:, 0, :, :d], cache[:, 1, :, :d] = k, v
    cache = cache.to(gpu)
    kv_, vv = cache[:, 0, :, :d], cache[:, 1, :, :d]
    outbuf = _sentinel((Tq, H, 2 * d), dtype, gpu)
    outv = outbuf[..., :d]
    assert not (qv.is_contiguous() or kv_.is_contiguous() or vv.is_contiguous() or outv.is_contiguous())
    assert kv_.stride() == vv.stride() == (4 * Hkv * d, 2 * d, 1)
    handle = L.lib()
    real, seen = handle.fa_fwd_varlen_kv, []

    def spy(*a):
        seen.append([x.value if isinstance(x, ctypes.c_void_p) else x for x in a[:7]] + [list(s) for s in a[15:18]])
        return real(*a)

    monkeypatch.setattr(handle, "fa_fwd_varlen_kv", spy)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with ops.launched_kernels() as kl:
        assert ops.attention_varlen(qv, kv_, vv, cqd, MSL_Q, causal=causal, out=outv, cu_seqlens_k=ckd,
                                    max_seqlen_k=MSL_K) is outv
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before, "the call allocated device memory (a copy?)"
    assert len(kl) == 1 and kl[0].startswith(_label(causal, True)), kl
    assert seen == [[qv.data_ptr(), kv_.data_ptr(), vv.data_ptr(), outv.data_ptr(), cqd.data_ptr(), ckd.data_ptr(), None,
                     [(H + 2 * Hkv) * d, d], [4 * Hkv * d, 2 * d], [2 * H * d, 2 * d]]], seen
    assert torch.equal(outv, want)
    assert (outbuf[..., d:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_kv_padded_head_dim(gpu, causal, dtype):
    """d = 80 has no kernel: zero-padded to 128 with the scale of d = 80."""
    from exploring_flash_attention_amd import ops
    pairs = ((1, 65), (65, 130), (0, 3), (130, 131), (20, 5))
    q, k, v, cu_q, cu_k = _kv_batch(80, 4, 2, dtype, 7, pairs)
    ref, owned = _kv_ref(80, 4, 2, dtype, causal, 130, 131, 7, pairs)
    out = _sentinel(q.shape, dtype, gpu)
    with ops.launched_kernels() as kl:
        ops.attention_varlen(q.to(gpu), k.to(gpu), v.to(gpu), _cu_dev(cu_q, gpu), 130, causal=causal, out=out,
                             cu_seqlens_k=_cu_dev(cu_k, gpu), max_seqlen_k=131)
    assert len(kl) == 1 and kl[0].startswith(_label(causal, True))
    own = torch.from_numpy(owned.copy())
    _gate(out.cpu()[own], ref[owned], dtype, f"kv padded d=80 causal={causal}")
    assert (out.cpu()[~own].float() == SENTINEL).all()


@pytest.mark.gpu
def test_varlen_kv_empty_inputs_and_restrictions(gpu):
    from exploring_flash_attention_amd import ops
    bf = torch.bfloat16
    q, kv = torch.ones(8, 4, 64, dtype=bf, device=gpu), torch.ones(20, 2, 64, dtype=bf, device=gpu)
    with ops.launched_kernels() as kl:
        e = torch.empty(0, 4, 64, dtype=bf, device=gpu)  # Tq = 0
        assert tuple(ops.attention_varlen(e, kv, kv, _cu_dev([0, 0], gpu), 64, cu_seqlens_k=_cu_dev([0, 20], gpu),
                                          max_seqlen_k=20).shape) == (0, 4, 64)
        out = _sentinel(q.shape, bf, gpu)
        ops.attention_varlen(q, kv, kv, _cu_dev([0], gpu), 64, out=out, cu_seqlens_k=_cu_dev([0], gpu),
                             max_seqlen_k=20)  # B = 0
        assert (out == SENTINEL).all()
    assert kl == []
    # Tk = 0 and max_seqlen_k = 0: no key anywhere, the rows of a sequence are zeros, the others kept
    ekv = torch.empty(0, 2, 64, dtype=bf, device=gpu)
    for kk, ck, mk in ((ekv, [0, 0], 5), (kv, [0, 20], 0)):
        out = _sentinel(q.shape, bf, gpu)
        ops.attention_varlen(q, kk, kk, _cu_dev([0, 6], gpu), 8, out=out, cu_seqlens_k=_cu_dev(ck, gpu), max_seqlen_k=mk)
        assert (out[:6] == 0).all() and (out[6:] == SENTINEL).all()
    w, wk = torch.zeros(8, 1, 384, dtype=bf, device=gpu), torch.zeros(9, 1, 384, dtype=bf, device=gpu)
    with pytest.raises(NotImplementedError, match="256"):
        ops.attention_varlen(w, wk, wk, _cu_dev([0, 8], gpu), 8, cu_seqlens_k=_cu_dev([0, 9], gpu), max_seqlen_k=9)
    f, fk = torch.zeros(8, 1, 64, dtype=torch.float64, device=gpu), torch.zeros(9, 1, 64, dtype=torch.float64, device=gpu)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.attention_varlen(f, fk, fk, _cu_dev([0, 8], gpu), 8, cu_seqlens_k=_cu_dev([0, 9], gpu), max_seqlen_k=9)
    with pytest.raises(ValueError, match="cu_seqlens_k"):  # a host cu_seqlens_k
        ops.attention_varlen(q, kv, kv, _cu_dev([0, 8], gpu), 8, cu_seqlens_k=torch.tensor([0, 20], dtype=torch.int32),
                             max_seqlen_k=20)
    with pytest.raises(ValueError, match="seqused_k"):  # a host seqused_k
        ops.attention_varlen(q, kv, kv, _cu_dev([0, 8], gpu), 8, cu_seqlens_k=_cu_dev([0, 20], gpu), max_seqlen_k=20,
                             seqused_k=torch.tensor([3], dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
def test_varlen_kv_graph_replay_follows_the_length_arrays(gpu, causal):
    """The call captured once on a side stream; cu_seqlens_k and seqused_k rewritten in place; the
    replay equals the eager result for the new lengths bit for bit (nothing was read at capture)."""
    from exploring_flash_attention_amd import ops
    dtype, d, H, Hkv, Lmax = torch.bfloat16, 128, 4, 2, 256
    g = torch.Generator().manual_seed(31)
    lens_q = (130, 40, 1)
    cu_q = _cu_dev(np.concatenate([[0], np.cumsum(lens_q)]), gpu)
    q = torch.randn(sum(lens_q), H, d, generator=g).to(dtype).to(gpu)
    k, v = (torch.randn(3 * Lmax, Hkv, d, generator=g).to(dtype).to(gpu) for _ in range(2))
    rounds = (([0, 256, 512, 768], [200, 40, 7]), ([0, 250, 300, 700], [256, 0, 90]), ([0, 100, 500, 768], [64, 130, 1]))
    cu_k, su = _cu_dev(rounds[0][0], gpu), _cu_dev(rounds[0][1], gpu)
    out = torch.empty_like(q)

    def call():
        return ops.attention_varlen(q, k, v, cu_q, 130, causal=causal, out=out, cu_seqlens_k=cu_k, max_seqlen_k=Lmax,
                                    seqused_k=su)

    wants = []
    for ck, s_ in rounds:
        wants.append(ops.attention_varlen(q, k, v, cu_q, 130, causal=causal, cu_seqlens_k=_cu_dev(ck, gpu),
                                          max_seqlen_k=Lmax, seqused_k=_cu_dev(s_, gpu)).clone())
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[1], wants[2])
    s = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    for (ck, s_), want in zip(rounds, wants):
        cu_k.copy_(_cu_dev(ck, gpu))
        su.copy_(_cu_dev(s_, gpu))
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (ck, s_)
