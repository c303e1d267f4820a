"""Softmax-weight readout of the causal, GQA, decode and paged-decode kernels.

The parity tests of test_causal.py / test_gqa.py / test_decode.py / test_decode_paged.py gate
|out - ref| <= A + eps * |ref| on random V: in a long row a single key's weight moves an output
element by about A or less, so a key dropped or admitted at a tile, split or page edge in one
row or lane can pass, and what they do catch they catch without saying which key.  This file
reads the weights themselves: every key of every row at relative precision, whatever n is.

The probe.  For a window start j0 the selector V[j, c] = 1 if j == j0 + c else 0 (c in [0, d),
exact in bf16 and fp16) makes O[i, c] = P[i, j0 + c], the softmax weight of key j0 + c; every
other key contributes an exact zero.  Every (b, h_kv) has its own q, k and its own window, and
the window index is rotated over ceil(Lk / d) calls, so every head's whole P matrix is read
(V belongs to the K/V head: the G query heads of a group read the same window).  The paged op
gets the selector scattered into the pool through a shuffled table, NaN wherever no table entry
points.

Reference: fp64 softmax weights on the storage-rounded q, k under each op's own mask (causal
lower triangle; head map h // G; decode's len_b = clamp(seqlens[b], 0, Lk) and the bottom-right
rule j <= len_b - Lq + i), cross-checked against causal_ref / gqa_ref / decode_ref to 1e-12.

Gate.  A masked or out-of-range key reads bitwise +-0 (a row without a visible key is all zero);
a visible one satisfies |out - P| <= K * eps * P + FLOOR with eps the half-ulp of GATE (2^-8
bf16, 2^-11 fp16), K = 4, FLOOR = 2^-120 (bf16), 2^-23 (fp16).  The kernels round P to the
storage type before P.V (one half-ulp) and round O once (a second); whether l is summed from the
rounded P (MFMA row sums) or the unrounded P (VALU sums) changes nothing at this order; fp16 P
below 2^-14 of the running max is subnormal (absolute error 2^-25) and so is an output below
2^-14 (the floor); the other two eps are margin for fp32 exp2, the l accumulation and the merges
of waves and splits.  test_emulation_stays_inside_the_bound holds a NumPy emulation of exactly
those steps (64-key tiles, four waves, the per-key causal tail with unrounded P, the base-2 lse
combine) to 0.75 of that bound; its worst err / bound over the three families, causal L = 384
and decode Lk = 1041 / 200: 0.50 (bf16), 0.50 (fp16).

Input families, their defining properties asserted on the CPU from the reference scores
(test_input_families_have_their_properties):
  flat   q, k ~ N(0, 1): every visible weight is near 1 / n (small weights, dropped keys, split
         weights).
  steep  q ~ 3 N(0, 1): the row maximum moves between tiles (asserted: in at least a third of
         the rows of 200 keys or more).  No row's visible scores span more than 40 log2 units
         (bf16 never meets its floor), and a head's visible scores span at least 20 natural
         units wherever the head has STEEP_MIN_SCORES of them.  Scores of deviation 3 leave the
         two bounds little room: n of them span about 6 sqrt(2 ln n), which is 20 only from some
         thousands on (a decode head of 3 x 200 scores or a sequence of 37 keys spans 13 to 19)
         and passes 40 log2 units = 27.7 when a whole head of 384 x 384 is taken together (28 to
         32); so the upper bound is taken per row, which is what one softmax spans (39.7 at
         most under the seeds' SALT), and the lower one per head with enough scores.
  tempt  the first key a row must not see carries that row's largest raw score (forward:
         k[j] = 1.5 q[j - 1], q scaled by 2, q of the group's first head; decode: key
         len_b - Lq + i + 1 aligned with q[b, h0, i], key len_b with the last row).  A leak, a
         maximum taken before the mask or a zero l turns whole rows wrong or non-finite.

test_readout_gate_rejects_what_the_output_gate_accepts plants four defects in the emulation (flat
inputs, causal L = 384 and decode Lk = 1041 in five splits) and asserts that this gate rejects
each: (1) the last visible key of rows >= 128 dropped, (2) key i + 1 admitted in rows >= 128,
(3) splits merged with e^lse on base-2 lse, (4) the row maximum taken before the mask on tempt
inputs (P underflows; fp16: l = 0 and whole rows are lost).  What the output gate of the parity
tests (A + eps |ref| and mean_rel on P @ V, V ~ N(0, 1)) says to the same outputs is printed,
and it is less blind than hoped: with EVERY row from 128 on hit it rejects (1) at 17 (bf16) / 53
(fp16) times its bound and (2) at 20 / 61 -- rows just past 128 hold weights up to 0.05 -- and it
rejects (3) through mean_rel (4e-2 against 1e-2) and at 1.8 / 5.8 times its bound, also with
whole splits of similar lse (3.5 / 11).  The gap it leaves is the defect confined to one row of
a late query tile: (1) in row 383 alone passes it in bf16 (0.73 of its bound; fp16, A = 2e-3,
still sees that 1.5e-3 |v|), which is asserted, and this gate rejects it at 64 times its bound.
(4) passes the output gate in bf16 (0.70) and fails it in fp16.

Two more are planted for the kernels test_weight_readout_fwd.py reads (full attention, flat
inputs): (5) a stale K tile at a chain seam -- the first 64 keys of head 1's first query tile
scored against head 0's K -- in all 128 rows of the tile and in row 5 alone: the readout rejects
both at thousands of times its bound (2e3 bf16, 1.5e4 fp16 for the single row); the output gate,
printed, rejects both too in either type (another head's weights are wrong by the whole weight,
not by one key's).  (6) In a ragged batch of 65 and 257 keys the last key of the longer sequence
dropped in its last row alone: rejected at 64 (bf16) / 510 (fp16) times the bound; the output
gate, printed and not asserted, rejects it in both types as well (one key of 257 is 4e-3 of v).

The many-head cases (chain_cases: the chained persistent kernels need a query tile per workgroup
of a two-per-compute-unit grid, so hundreds of heads share a seed) take q ~ 2.5 N(0, 1) for
steep: with 3 N(0, 1) the largest row span over so many rows is 43 to 46 log2 units, past the
cap.  Asserted for their seeds at 256 compute units: no row spans more than 40 log2 units
(measured 33.6 to 36.1) and the row maximum moves between 64-key tiles in at least a third of the
rows; the per-head spread is not bounded there (measured minimum 19.5 natural units).

Split-KV partial formats (attention_v2; split_extra, emulate_v2).  fp32 partials pass the bound
as it stands.  A 16-bit partial is one more rounding of x = P / f, f the split's share of the
row, which the combine scales back by f.  Scaled fp16 (x * 2^-e, 2^e <= 2 max x over the row's
partial, with a selector V the probed window inside the split): a relative half-ulp 2^-11 above
2^-14 (inside K), half the subnormal spacing below it, 2^-25 * 2^e <= 2^-24 max x, so the bound
is K eps P + FLOOR + c * 2^-24 * max(P over window and split), c = 2 (the worst case doubled, as K
doubles its two half-ulps).  The input type unscaled: K eps P + FLOOR + eps P (+ 2^-25, fp16
subnormals).  test_split_kv_emulation_stays_inside_the_bound holds emulate_v2 (per-split
normalised partial, the rounding to the format, {lse, e}, the base-2 combine) to 0.75 of these.

Measured on an MI355X, worst err / bound over all cases and families (emulation beside it):
                              bf16          fp16
  causal forward              0.59 (0.50)   0.51 (0.50)
  GQA forward                 0.60          0.54
  decode                      0.50 (0.50)   0.49 (0.47)
  paged decode                0.50          0.47          (bitwise the contiguous decode)
  full forward                0.56 (0.50)   0.52 (0.49)   (the strided forms: 0.56, 0.50)
  chain <final>, <final, gqa> 0.60          0.56
  split-KV one-shot  fp32     0.59 (0.51)   0.54 (0.48)
                     input    0.61 (0.57)   0.57 (0.54)
                     scaled   0.59 (0.50)   0.71 (0.67)
  split-KV arrive-first       0.50 / 0.57 / 0.51   0.45 / 0.53 / 0.66   (fp32 / input / scaled)
  split-KV <fused walk>       0.58 / 0.60 / 0.58   0.52 / 0.58 / 0.72   (scaled: the walk; the others one-shot)
  varlen                      0.58          0.54
  d-tiled d = 384             0.50 (0.50)   0.48 (0.48)   (padded d = 300: 0.50)
  d-tiled d = 512 <paired>    0.51 (0.51)   0.51 (0.51)   (padded d = 400: 0.49)
  raw partial        fp32     0.43 (0.42)   0.43 (0.39)   (against the shard-local weights; the
                     input    0.52 (0.53)   0.52 (0.48)    strided q forms included; bounds:
                     scaled   0.48 (0.48)   0.69 (0.64)    test_weight_readout_partial.py)
  partial lse                 0.13 (0.08)   0.13 (0.09)   (every format alike)
  combine            fp32     0.50 (0.49)   0.48 (0.47)
                     input    0.56 (0.54)   0.56 (0.54)
                     scaled   0.52 (0.50)   0.70 (0.67)
No kernel left the bound; the decode figures at Lk = 1041 are those of the emulation to three
digits.  (The emulations of the last nine rows run on fewer cases than the kernels: L = 130 and
600 of the d-tiled lengths, the first and the last of the partial cases.)

Four more defects are planted for the kernels test_weight_readout_dtiled.py and
test_weight_readout_partial.py read, each rejected by this gate; the output gate's verdict is
printed and rejects them too at these shapes (a few hundred keys at most: one weight is not small
there).  d-tiled wave pairs (d = 512, L = 600, emulate_dtiled_pair): (7) on the tile where a row
of wave 1 rose most (2^7.8, steep) wave 0 misses its partner's alpha, in every row of the wave and
in that row alone: the keys of the earlier tiles in wave 0's half of the columns are overweighted,
1.5e4 (bf16) / 1.1e5 (fp16) times the bound; (8) the partner's row sum taken from the wave's own
row of the same index (flat): 68 / 530 times the bound.  Partial and combine (flat, d = 64, Lk =
193 in shards of 64 keys, emulate_partial_combine): (9) the last key of the last shard, a shard
of that one key, dropped in the last row of each chunk: the raw partial reads 0 for a weight of
1, 64 to 85 (bf16) / 510 to 680 (fp16) times its bound, the combined row 51 to 64 / 410 to 510;
(10) the combine decoding row r's scaled partial with the exponent of row r ^ 1: 450 / 3600.
"""
import functools
import itertools
import zlib

import numpy as np
import pytest
import torch

from test_causal import causal_ref
from test_decode import DTYPES, GATE, IDS, _bits, _sl, decode_ref
from test_decode import _gate as output_gate
from test_decode_paged import _perm_table
from test_gqa import gqa_ref

K_ULP = 4
FLOOR = {torch.bfloat16: 2.0 ** -120, torch.float16: 2.0 ** -23}
FAMILIES = ("flat", "steep", "tempt")
TILE = 64
LOG2E = 1.4426950408889634
STEEP_MIN_SCORES = 8000  # visible scores of a head from which a spread of 20 natural units is asserted

# (B, H, d, L): B * H >= ceil(L / d), so one call already touches every window
CAUSAL_CASES = ([(2, 3, d, L_) for d in (64, 128) for L_ in (65, 129, 200, 384)]
                + [(2, 4, 32, 200), (2, 3, 256, 160)])
GQA_HEADS = ((2, 4, 2), (1, 4, 1))
GQA_SHAPES = [(d, L_) for d in (64, 128) for L_ in (200, 384)]
DECODE_HEADS = ((4, 2, 3), (8, 1, 8), (4, 2, 13), (2, 2, 64))  # (H, H_kv, Lq)
DECODE_LENS = (None, (200, 37), (130, 5))
DECODE_SPLITS = (None, 1, 3)
LONG = dict(B=2, H=8, Hkv=1, Lq=8, Lk=1041, ns=5, lens=(1027, 37))  # tail keys 1020..1026 over the edge at 1024
PAGES = (64, 128)


# ----------------------------------------------------------------------------------------
# inputs, reference weights, the selector
# ----------------------------------------------------------------------------------------


SALT = 7  # of the seeds: the steep family's two bounds leave 3 * N(0, 1) little room (see the docstring)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr((SALT,) + key).encode()))


def _lens(seqlens, B, Lk):
    return [Lk if seqlens is None else min(max(int(seqlens[b]), 0), Lk) for b in range(B)]


@functools.lru_cache(maxsize=None)
def fwd_inputs(family, B, H, Hkv, L_, d, dtype):
    """Storage-rounded q [B, H, L, d], k [B, H_kv, L, d] of a forward case; nobody writes to them."""
    g = _gen("fwd", family, B, H, Hkv, L_, d)
    q = torch.randn(B, H, L_, d, generator=g) * {"flat": 1.0, "steep": 3.0, "tempt": 2.0}[family]
    k = torch.randn(B, Hkv, L_, d, generator=g)
    q = q.to(dtype)
    if family == "tempt":  # key j is aligned with row j - 1 of the group's first head
        k[:, :, 1:] = 1.5 * q[:, ::H // Hkv, :-1].float()
    return q, k.to(dtype)


MANY_HEAD_STEEP = 2.5  # q scale of `steep` where hundreds of heads share a seed (see the docstring)
MI355X_CUS = 256       # the CPU tests size the chain cases for this device; the GPU tests ask the device


def chain_cases(cus):
    """{name: (H, H_kv, L)} at B = 1, d = 128, of the chained persistent kernels' readout on a
    device of `cus` compute units (grid = 2 * cus // 8 * 8 workgroups, fa_fwd.hip's launch rule):
    one-item: a query tile per workgroup; uneven: some workgroups run two items and the item count
    is no multiple of 8; cross-head: three query tiles per head, six key tiles per item, lists that
    cross head boundaries; gqa: the uneven case with G = 4; walk / walk-uneven: attention_v2's
    chained walk over two 256-key blocks, four query tiles per head."""
    grid = 2 * cus // 8 * 8
    uneven = grid // 2 + grid // 8 + 3
    return {"one-item": (grid // 2, grid // 2, 256), "uneven": (uneven, uneven, 256),
            "cross-head": (-(-grid // 3) + 5,) * 2 + (384,), "gqa": (-(-uneven // 4) * 4, -(-uneven // 4), 256),
            "walk": (grid // 4, grid // 4, 512), "walk-uneven": (grid // 4 + 3, grid // 4 + 3, 512)}


@functools.lru_cache(maxsize=None)
def many_head_inputs(family, H, Hkv, L_, d, dtype):
    """Storage-rounded q [1, H, L, d], k [1, H_kv, L, d] of a many-head case (flat / steep)."""
    g = _gen("many", family, H, Hkv, L_, d)
    q = torch.randn(1, H, L_, d, generator=g) * {"flat": 1.0, "steep": MANY_HEAD_STEEP}[family]
    k = torch.randn(1, Hkv, L_, d, generator=g)
    return q.to(dtype), k.to(dtype)


def head_chunks(q, k, step=32):
    """(h0, h1, q[:, h0:h1], k of those heads' K/V heads) in chunks of at most `step` query heads
    (a multiple of the group size), so that no fp64 [heads, L, L] array grows past ~100 MB."""
    H, Hkv = q.shape[1], k.shape[1]
    G = H // Hkv
    step = max(step // G, 1) * G
    for h0 in range(0, H, step):
        h1 = min(h0 + step, H)
        yield h0, h1, q[:, h0:h1], k[:, h0 // G:-(-h1 // G)]


@functools.lru_cache(maxsize=None)
def decode_inputs(family, B, H, Hkv, Lq, Lk, d, dtype, seqlens):
    """Storage-rounded q [B, H, Lq, d], k [B, H_kv, Lk, d] of a decode case."""
    g = _gen("decode", family, B, H, Hkv, Lq, Lk, d, seqlens)
    q = torch.randn(B, H, Lq, d, generator=g) * {"flat": 1.0, "steep": 3.0, "tempt": 2.0}[family]
    k = torch.randn(B, Hkv, Lk, d, generator=g)
    q = q.to(dtype)
    if family == "tempt":
        G = H // Hkv
        for b, n in enumerate(_lens(seqlens, B, Lk)):
            for i in range(Lq):  # the first key row position i must not see under the causal rule
                j = n - Lq + i + 1
                if 0 <= j < Lk:  # (i = Lq - 1: key len_b, also the first one past a non-causal row)
                    k[b, :, j] = 1.5 * q[b, ::G, i].float()
    return q, k.to(dtype)


def _softmax(s, vis):
    """fp64 weights of the visible keys, exact zeros elsewhere (a row without one: all zero)."""
    s = np.where(vis, s, -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    p = np.exp(s - np.where(np.isfinite(mx), mx, 0.0))
    l = p.sum(axis=-1, keepdims=True)
    return np.where(l > 0, p / np.where(l > 0, l, 1.0), 0.0)


def _scores(q, k):
    """Natural-unit fp64 scores [B, H, Lq, Lk] of storage tensors, head h against K/V head h // G."""
    qn, kn = q.double().numpy(), k.double().numpy()
    H, Hkv = qn.shape[1], kn.shape[1]
    kn = kn[:, np.arange(H) // (H // Hkv)]
    return qn @ np.swapaxes(kn, -1, -2) / np.sqrt(qn.shape[-1])


def fwd_weights(q, k, causal):
    """(P, vis, s): P [B, H, L, L] fp64, vis broadcastable to it."""
    s = _scores(q, k)
    L_ = s.shape[-1]
    vis = np.tril(np.ones((L_, L_), bool)) if causal else np.ones((L_, L_), bool)
    vis = np.broadcast_to(vis, s.shape)
    return _softmax(s, vis), vis, s


def decode_vis(B, Lq, Lk, seqlens, causal):
    vis = np.zeros((B, 1, Lq, Lk), bool)
    j = np.arange(Lk)
    for b, n in enumerate(_lens(seqlens, B, Lk)):
        for i in range(Lq):
            vis[b, 0, i] = (j < n) & ((j <= n - Lq + i) if causal else True)
    return vis


def decode_weights(q, k, seqlens, causal):
    s = _scores(q, k)
    vis = np.broadcast_to(decode_vis(s.shape[0], s.shape[2], s.shape[3], seqlens, causal), s.shape)
    return _softmax(s, vis), vis, s


def _windows(Lk, d):
    return -(-Lk // d)


def selector(B, Hkv, Lk, d, r, dtype):
    """V [B, H_kv, Lk, d] of rotation r: head n = b * H_kv + h_kv reads window (n + r) % windows."""
    nw = _windows(Lk, d)
    v = torch.zeros(B, Hkv, Lk, d, dtype=dtype)
    for n in range(B * Hkv):
        j0 = (n + r) % nw * d
        c = torch.arange(min(d, Lk - j0))
        v[n // Hkv, n % Hkv, j0 + c, c] = 1
    return v


def read_all(call, B, H, Hkv, Lq, Lk, d, dtype):
    """call(v) -> out [B, H, Lq, d] for every rotation; the outputs put in key order:
    [B, H, Lq, windows * d] (host, storage type)."""
    nw, G = _windows(Lk, d), H // Hkv
    got = torch.full((B, H, Lq, nw * d), float("nan"), dtype=dtype)
    for r in range(nw):
        out = call(selector(B, Hkv, Lk, d, r, dtype))
        out = out.cpu() if isinstance(out, torch.Tensor) else out
        assert out.dtype == dtype and tuple(out.shape) == (B, H, Lq, d)
        for n in range(B * Hkv):
            b, h0, w = n // Hkv, n % Hkv * G, (n + r) % nw
            got[b, h0:h0 + G, :, w * d:(w + 1) * d] = out[b, h0:h0 + G]
    return got


def _pad_keys(x, n):
    return np.concatenate([x, np.zeros(x.shape[:-1] + (n - x.shape[-1],), x.dtype)], axis=-1)


def readout_check(got, P, vis, dtype, extra=None, k_ulp=K_ULP):
    """(masked elements that are not +-0, non-finite elements, worst err / bound over the visible
    ones) of a readout `got` [..., n >= Lk] (host; the storage type, or float32: a decoded fp32 or
    scaled split-KV partial, its +-0 test on the float32 bit pattern) against fp64 weights P
    [..., Lk].  extra [..., Lk]: a derived term added to the bound K eps P + FLOOR (the 16-bit
    split-KV partial formats, split_extra); None: the bound as it stands.  k_ulp: K (K_ULP - 1
    for a partial stored without the output's rounding, test_weight_readout_partial.py)."""
    n = got.shape[-1]
    P, vis = _pad_keys(P, n), _pad_keys(np.ascontiguousarray(vis), n)
    extra = 0.0 if extra is None else _pad_keys(np.ascontiguousarray(extra, np.float64), n)
    if got.dtype == torch.float32:
        nonzero = (got.contiguous().view(torch.int32).numpy() & 0x7FFFFFFF) != 0
    else:
        nonzero = (got.contiguous().view(torch.int16).numpy() & 0x7FFF) != 0
    x = got.double().numpy()
    assert x.shape == P.shape, (x.shape, P.shape)
    leaked = int(nonzero[~vis].sum())
    bad = int((~np.isfinite(x)).sum())
    with np.errstate(invalid="ignore"):
        ratio = (np.abs(x - P) / (k_ulp * GATE[dtype][2] * P + FLOOR[dtype] + extra))[vis]
    worst = float(np.where(np.isfinite(ratio), ratio, np.inf).max()) if ratio.size else 0.0
    return leaked, bad, worst


def readout_gate(got, P, vis, dtype, label, limit=1.0, quiet=False, extra=None, k_ulp=K_ULP):
    leaked, bad, worst = readout_check(got, P, vis, dtype, extra, k_ulp)
    if not quiet:
        print(f"readout {label}: worst err/bound={worst:.3f}")
    assert leaked == 0, (label, f"{leaked} masked or out-of-range keys read nonzero")
    assert bad == 0, (label, f"{bad} non-finite weights")
    assert worst <= limit, (label, worst)
    return worst


# ----------------------------------------------------------------------------------------
# the emulation: the rounding steps of the kernels in NumPy (fp32 arithmetic)
# ----------------------------------------------------------------------------------------


def _round_to(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dtype).float().numpy()


def _exp2_diff(a, b):
    """2^(a - b) in fp32, 0 where a is -inf (also against b = -inf)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(a), np.float32(0), np.exp2(a - np.where(np.isneginf(b), np.float32(0), b))).astype(np.float32)


class _State:
    """(m, l, acc) of the online softmax over R rows; acc[i, j] is the weight of key j so far."""

    def __init__(self, R, n):
        self.m = np.full(R, -np.inf, np.float32)
        self.l = np.zeros(R, np.float32)
        self.acc = np.zeros((R, n), np.float32)

    def fold(self, s2, cols, dtype, smax=None):
        """Keys `cols` (a slice) of the masked base-2 scores s2 [R, n] (-inf: masked).  dtype: P is
        rounded to it before it is summed and used (the MFMA tiles); None: P stays fp32 (the
        per-key VALU path).  smax: the scores the tile's row maximum is taken from (defect 4)."""
        mx = (s2 if smax is None else smax)[:, cols].max(axis=1)
        m_new = np.maximum(self.m, mx)
        alpha = _exp2_diff(self.m, m_new)
        p = _exp2_diff(s2[:, cols], m_new[:, None])
        if dtype is not None:
            p = _round_to(p, dtype)
        self.m = m_new
        self.l = self.l * alpha + p.sum(axis=1, dtype=np.float32)
        self.acc *= alpha[:, None]
        self.acc[:, cols] = p

    def merge(self, other):
        m_new = np.maximum(self.m, other.m)
        w1, w2 = _exp2_diff(self.m, m_new), _exp2_diff(other.m, m_new)
        self.m = m_new
        self.l = self.l * w1 + other.l * w2
        self.acc = self.acc * w1[:, None] + other.acc * w2[:, None]

    def normalised(self):
        inv = np.where(self.l > 0, np.float32(1) / np.where(self.l > 0, self.l, np.float32(1)), np.float32(0))
        return self.acc * inv[:, None]


def _base2(s, vis, d):
    """Masked base-2 fp32 scores of natural fp64 scores (the kernels' s * scale * log2 e)."""
    return np.where(vis, (s * LOG2E).astype(np.float32), np.float32(-np.inf))


def emulate_forward(s2, dtype, smax=None):
    """One query tile against 64-key tiles in order: P rounded to the storage type, l from the
    rounded P, the output rounded.  s2 [R, n].  Returns (weights fp32 before the output rounding,
    the output as a storage tensor)."""
    st = _State(*s2.shape)
    for t0 in range(0, s2.shape[1], TILE):
        st.fold(s2, slice(t0, min(t0 + TILE, s2.shape[1])), dtype, smax)
    w = st.normalised()
    return w, torch.from_numpy(w).to(dtype)


SCALED_C = 2
PARTIAL_FORMATS = ("fp32", "input", "scaled")  # torch.float32, the input dtype, ops.PARTIAL_FP16_SCALED


def _segments(Lk, d, kps):
    """Starts of the key segments (probed window) x (key split): both edge sets."""
    return np.array(sorted(set(range(0, Lk, d)) | set(range(0, Lk, kps))))


def split_extra(P, d, kps, fmt, dtype):
    """What a 16-bit split-KV partial format adds to K eps P + FLOOR, from the format alone.  A
    split's normalised partial row is x = P / f (f the split's share of the row) over the keys of
    the probed window inside the split, and the combine scales its error back by f.
    scaled: x * 2^-e is stored as fp16 with 2^e <= 2 max(x): above 2^-14 a relative half-ulp 2^-11
      (fp16 inputs: one of K's two spare eps; bf16: an eighth of one), below it half the subnormal
      spacing, an absolute 2^-25 * 2^e <= 2^-24 max(x), reached when max(x) sits just above a power
      of two: c * 2^-24 * max(P over window and split) with c = SCALED_C = 2, the worst case
      doubled as K doubles the two half-ulps it is derived from (so that the emulation, which
      meets the worst case at the smallest weights, stays at half the bound as it does there).
    input: x stored as bf16 / fp16: one more half-ulp, eps P, and for fp16 the subnormal 2^-25.
    fp32: nothing (None)."""
    if fmt == "fp32":
        return None
    if fmt == "input":
        return GATE[dtype][2] * P + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    seg = _segments(P.shape[-1], d, kps)
    mx = np.maximum.reduceat(P, seg, axis=-1)
    return SCALED_C * 2.0 ** -24 * np.repeat(mx, np.diff(np.append(seg, P.shape[-1])), axis=-1)


def emulate_v2(s2, d, kps, fmt, dtype):
    """attention_v2 on one query tile's rows, s2 [R, Lk] base-2 scores: per split of kps keys the
    forward's 64-key tiles (P rounded, l from the rounded P), the normalised partial rounded to
    the partial format -- scaled: per probed window of d keys (what one call's partial row holds)
    times 2^-e, e the exponent of the row's largest value, to fp16 -- its {lse, e}, and the
    base-2 combine in split order.  Returns (weights fp32, output storage tensor)."""
    R, Lk = s2.shape
    parts, lses = [], []
    for k0 in range(0, Lk, kps):
        st = _State(R, Lk)
        for t0 in range(k0, min(k0 + kps, Lk), TILE):
            st.fold(s2, slice(t0, min(t0 + TILE, k0 + kps, Lk)), dtype)
        part = st.normalised()
        if fmt == "input":
            part = _round_to(part, dtype)
        elif fmt == "scaled":
            for w0 in range(0, Lk, d):
                cols = slice(max(w0, k0), min(w0 + d, k0 + kps, Lk))
                if cols.start >= cols.stop:
                    continue
                e = np.frexp(part[:, cols].max(axis=1))[1][:, None]  # max * 2^-e in [0.5, 1); 0 -> e = 0
                part[:, cols] = np.ldexp(_round_to(np.ldexp(part[:, cols], -e), torch.float16), e)
        parts.append(part)
        with np.errstate(divide="ignore"):
            lses.append(np.where(st.l > 0, st.m + np.log2(st.l), -np.inf).astype(np.float32))
    M = np.max(lses, axis=0)
    acc, wsum = np.zeros((R, Lk), np.float32), np.zeros(R, np.float32)
    for part, lse in zip(parts, lses):
        wgt = _exp2_diff(lse, M)
        acc += wgt[:, None] * part
        wsum += wgt
    w = acc * (np.float32(1) / wsum)[:, None]
    return w, torch.from_numpy(w).to(dtype)


def emulate_decode(s2, n, Lq, causal, kps, dtype, natural_merge=False):
    """One (b, h_kv) group of the decode kernel: s2 [R, Lk] masked base-2 scores, n = len_b.  Per
    split four waves take the 64-key tiles t = w, w + 4, ... below the causal tail with rounded
    P and then every fourth key of the tail one at a time with unrounded P; the waves are merged in
    order; one split: the output is rounded; several: a normalised fp32 partial and a base-2 lse,
    combined with weights 2^(lse - max) (natural_merge: e^(lse - max), defect 3)."""
    R, Lk = s2.shape
    nsplit = -(-Lk // kps)
    all_end = max(n - Lq + 1, 0) if causal else n
    parts, lses = [], []
    for s in range(nsplit):
        kv_begin, kv_end = s * kps, min(s * kps + kps, n)
        if kv_begin >= n:
            parts.append(np.zeros((R, Lk), np.float32))
            lses.append(np.full(R, -np.inf, np.float32))
            continue
        mf_end = min(kv_end, all_end)
        nt = -(-(mf_end - kv_begin) // TILE) if mf_end > kv_begin else 0
        waves = [_State(R, Lk) for _ in range(4)]
        for w, st in enumerate(waves):
            for t in range(w, nt, 4):
                st.fold(s2, slice(kv_begin + t * TILE, min(kv_begin + (t + 1) * TILE, mf_end)), dtype)
            if causal and Lq > 1:
                for j in range(max(kv_begin, all_end) + w, kv_end, 4):
                    st.fold(s2, slice(j, j + 1), None)
        for st in waves[1:]:
            waves[0].merge(st)
        parts.append(waves[0].normalised())
        with np.errstate(divide="ignore"):
            lses.append(np.where(waves[0].l > 0, waves[0].m + np.log2(waves[0].l), -np.inf).astype(np.float32))
    if nsplit == 1:
        return parts[0], torch.from_numpy(parts[0]).to(dtype)
    M = np.max(lses, axis=0)
    acc, wsum = np.zeros((R, Lk), np.float32), np.zeros(R, np.float32)
    for part, lse in zip(parts, lses):
        wgt = _exp2_diff(lse, M)
        if natural_merge:
            wgt = (wgt ** np.float32(LOG2E)).astype(np.float32)  # e^(lse - M) = (2^(lse - M))^(log2 e)
        acc += wgt[:, None] * part
        wsum += wgt
    w = acc * np.where(wsum > 0, np.float32(1) / np.where(wsum > 0, wsum, np.float32(1)), np.float32(0))[:, None]
    return w, torch.from_numpy(w).to(dtype)


def emulate_decode_case(q, k, seqlens, causal, kps, dtype, natural_merge=False):
    """emulate_decode over every group of a decode case; (weights fp32, output) [B, H, Lq, Lk]."""
    B, H, Lq, d = q.shape
    Hkv, Lk = k.shape[1], k.shape[2]
    G = H // Hkv
    _, vis, s = decode_weights(q, k, seqlens, causal)
    s2 = _base2(s, vis, d)
    w = np.zeros(s.shape, np.float32)
    for b, n in enumerate(_lens(seqlens, B, Lk)):
        for hkv in range(Hkv):
            rows = s2[b, hkv * G:(hkv + 1) * G].reshape(G * Lq, Lk)
            w[b, hkv * G:(hkv + 1) * G] = emulate_decode(rows, n, Lq, causal, kps, dtype, natural_merge)[0].reshape(G, Lq, Lk)
    return w, torch.from_numpy(w).to(dtype)


def _plan_kps(c):
    from exploring_flash_attention_amd import ops
    return ops.decode_plan(c["B"], c["H"], c["Hkv"], c["Lq"], c["Lk"], 64, c["ns"], cus=256)[1]


# ----------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------


def test_reference_weights_match_the_output_references():
    """The weights of this file times a random fp64 V are causal_ref / gqa_ref / decode_ref."""
    g = torch.Generator().manual_seed(5)
    B, H, Hkv, L_, d = 2, 6, 2, 37, 16
    q = torch.randn(B, H, L_, d, generator=g, dtype=torch.float64)
    k, v = (torch.randn(B, Hkv, L_, d, generator=g, dtype=torch.float64) for _ in range(2))
    ve = v.numpy()[:, np.arange(H) // (H // Hkv)]
    for causal in (False, True):
        P, vis, _ = fwd_weights(q, k, causal)
        assert np.abs(P @ ve - gqa_ref(q.numpy(), k.numpy(), v.numpy(), causal)).max() <= 1e-12, causal
        assert (P[~vis] == 0).all() and np.abs(P.sum(-1) - 1).max() <= 1e-12
    kf, vf = (torch.randn(B, H, L_, d, generator=g, dtype=torch.float64) for _ in range(2))
    P, _, _ = fwd_weights(q, kf, True)
    assert np.abs(P @ vf.numpy() - causal_ref(q.numpy(), kf.numpy(), vf.numpy())).max() <= 1e-12
    Lq, Lk = 4, 23
    qd = q[:, :, :Lq]
    kd, vd = (torch.randn(B, Hkv, Lk, d, generator=g, dtype=torch.float64) for _ in range(2))
    ve = vd.numpy()[:, np.arange(H) // (H // Hkv)]
    for seqlens, causal in itertools.product((None, (23, 9), (2, 40), (0, 3)), (False, True)):
        P, vis, _ = decode_weights(qd, kd, seqlens, causal)
        want = decode_ref(qd.numpy(), kd.numpy(), vd.numpy(), seqlens, causal)
        assert np.abs(P @ ve - want).max() <= 1e-12, (seqlens, causal)
        assert (P[~vis] == 0).all()
        rows = vis.any(-1)
        assert np.abs(P.sum(-1)[rows] - 1).max() <= 1e-12 and (P[~rows] == 0).all()
    assert not decode_vis(2, 4, 23, (2, 40), True)[0, 0, :2].any()  # len 2 < Lq 4: rows 0, 1 see nothing


def _all_cases():
    """(op, family, dtype, q, k, vis, s, tempt rows): every input set of the GPU tests."""
    for family, dtype in itertools.product(FAMILIES, DTYPES):
        for B, H, d, L_ in CAUSAL_CASES:
            q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
            yield ("causal", family, dtype, (B, H, H, L_, L_, d, None, True), q, k) + fwd_weights(q, k, True)[1:]
        for (B, H, Hkv), (d, L_), causal in itertools.product(GQA_HEADS, GQA_SHAPES, (False, True)):
            q, k = fwd_inputs(family, B, H, Hkv, L_, d, dtype)
            yield ("gqa", family, dtype, (B, H, Hkv, L_, L_, d, None, causal), q, k) + fwd_weights(q, k, causal)[1:]
        for (H, Hkv, Lq), d, lens, causal in itertools.product(DECODE_HEADS, (64, 128), DECODE_LENS, (False, True)):
            q, k = decode_inputs(family, 2, H, Hkv, Lq, 200, d, dtype, lens)
            yield ("decode", family, dtype, (2, H, Hkv, Lq, 200, d, lens, causal), q, k) + decode_weights(q, k, lens, causal)[1:]
        c = LONG
        for d, causal in itertools.product((64, 128), (False, True)):
            q, k = decode_inputs(family, c["B"], c["H"], c["Hkv"], c["Lq"], c["Lk"], d, dtype, c["lens"])
            yield (("decode", family, dtype, (c["B"], c["H"], c["Hkv"], c["Lq"], c["Lk"], d, c["lens"], causal), q, k)
                   + decode_weights(q, k, c["lens"], causal)[1:])


def _moving_max_rows(s, vis):
    """Rows whose running maximum rises in a 64-key tile after the first one with a visible key."""
    sm = np.where(vis, s, -np.inf)
    run = np.full(s.shape[:-1], -np.inf)
    moved = np.zeros(s.shape[:-1], bool)
    for t0 in range(0, s.shape[-1], TILE):
        mx = sm[..., t0:t0 + TILE].max(-1)
        moved |= np.isfinite(run) & (mx > run)
        run = np.maximum(run, mx)
    return moved


def test_input_families_have_their_properties():
    reached = {}
    for op, family, dtype, shape, q, k, vis, s in _all_cases():
        B, H, Hkv, Lq, Lk, d, lens, causal = shape
        G = H // Hkv
        label = (op, family, IDS[dtype], shape)
        sm_hi, sm_lo = np.where(vis, s, -np.inf), np.where(vis, s, np.inf)
        assert np.isfinite(s).all() and np.abs(s).max() < 1e3, label  # nothing near the end of fp32
        if family == "flat":
            # every visible weight within e^(+-8) of 1 / n (N(0, 1) scores stay inside +-6 over
            # the 1e6 of a case): no key of a row is negligible
            P = _softmax(s, vis)
            off = float(np.abs(np.log(np.where(vis, P * vis.sum(-1, keepdims=True), 1.0))).max())
            assert off < 8, (label, off)
        elif family == "steep":
            count = vis.sum(axis=(-1, -2))  # per (b, h)
            spread = np.where(count > 0, sm_hi.max(axis=(-1, -2)) - sm_lo.min(axis=(-1, -2)), 0.0)
            rows = np.where(vis.any(-1), sm_hi.max(-1) - sm_lo.min(-1), 0.0)  # what one softmax spans
            assert rows.max() * LOG2E <= 40, (label, float(rows.max() * LOG2E))
            assert (spread[count >= STEEP_MIN_SCORES] >= 20).all(), (label, spread, count)
            long_rows = vis.sum(-1) >= 200  # (the maximum of n keys sits past the first tile in 1 - 64 / n of the rows)
            if long_rows.any():
                assert _moving_max_rows(s, vis)[long_rows].mean() >= 1 / 3, label
            key = (op, IDS[dtype])
            reached[key] = max(reached.get(key, 0.0), float(spread.max()))
        else:
            h0 = np.arange(Hkv) * G  # the first query head of each group
            if op in ("causal", "gqa"):
                if not causal:
                    continue  # the full forward sees key i + 1: the inputs are merely peaked there
                i = np.arange(Lq - 1)
                tempt = s[:, h0][:, :, i, i + 1]
                seen = sm_hi[:, h0][:, :, :-1].max(-1)
                assert (tempt > seen).all(), (label, int((tempt <= seen).sum()))
                assert not vis[:, h0][:, :, i, i + 1].any()
            else:
                checked = 0
                for b, n in enumerate(_lens(lens, B, Lk)):
                    for i in range(Lq):
                        j = n - Lq + i + 1 if causal or i == Lq - 1 else -1
                        if not 0 <= j < Lk:
                            continue
                        assert not vis[b, h0, i, j].any(), label
                        if vis[b, 0, i].any():
                            assert (s[b, h0, i, j] > sm_hi[b, h0, i].max(-1)).all(), (label, b, i, j)
                        checked += 1
                assert checked > 0 or (lens is None and not causal), label
    assert all(v >= 20 for v in reached.values()), reached
    # the many-head cases (q ~ MANY_HEAD_STEEP N(0, 1)), sized for an MI355X, in head chunks: the
    # row cap and the moving maximum; the per-head spread is printed, not bounded
    least = {}
    for (name, (H, Hkv, L_)), dtype in itertools.product(chain_cases(MI355X_CUS).items(), DTYPES):
        span, moved, rows, spread = 0.0, 0, 0, np.inf
        for _, _, qc, kc in head_chunks(*many_head_inputs("steep", H, Hkv, L_, 128, dtype)):
            s = _scores(qc, kc)
            assert np.isfinite(s).all() and np.abs(s).max() < 1e3, (name, IDS[dtype])
            span = max(span, float((s.max(-1) - s.min(-1)).max()) * LOG2E)
            mv = _moving_max_rows(s, np.ones(s.shape, bool))
            moved, rows = moved + int(mv.sum()), rows + mv.size
            spread = min(spread, float((s.max(axis=(-1, -2)) - s.min(axis=(-1, -2))).min()))
        assert span <= 40, (name, IDS[dtype], span)
        assert moved >= rows / 3, (name, IDS[dtype], moved, rows)
        least[name, IDS[dtype]] = (round(span, 1), round(spread, 1))
    print("many-head steep (largest row span in log2 units, least per-head spread in natural units):", least)


EMU_FWD = (1, 2, 64, 384)  # B, H, d, L: six query tiles' worth of rows, six key tiles


def _emu_forward_case(family, dtype, defect=None, rows_from=128, rows_to=None):
    """The causal forward emulation at EMU_FWD; defect: 'drop' (the last visible key of rows
    rows_from..rows_to is masked), 'admit' (key i + 1 of those rows is not), 'premax' (the tile's
    row maximum is taken before the causal mask).  Returns (P, vis, weights fp32, output)."""
    B, H, d, L_ = EMU_FWD
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    P, vis, s = fwd_weights(q, k, True)
    kvis = np.array(vis)
    i = np.arange(rows_from, L_ if rows_to is None else rows_to)
    if defect == "drop":
        kvis[..., i, i] = False
    elif defect == "admit":
        i = i[i + 1 < L_]
        kvis[..., i, i + 1] = True
    s2 = _base2(s, kvis, d).reshape(B * H * L_, L_)
    smax = None
    if defect == "premax":  # unmasked inside the tiles a row visits (up to the one on its diagonal)
        row = np.arange(L_)[:, None]
        visited = np.arange(L_)[None, :] < (row // TILE + 1) * TILE
        smax = _base2(s, np.broadcast_to(visited, s.shape), d).reshape(B * H * L_, L_)
    w, out = emulate_forward(s2, dtype, smax)
    return P, vis, w.reshape(s.shape), out.reshape(s.shape)


def _emu_decode_case(family, dtype, causal=True, natural_merge=False, lens=LONG["lens"]):
    """The decode emulation at LONG (Lk = 1041 in five splits of 256 keys)."""
    c = LONG
    kps = _plan_kps(c)
    assert kps == 256 and -(-c["Lk"] // kps) == 5
    q, k = decode_inputs(family, c["B"], c["H"], c["Hkv"], c["Lq"], c["Lk"], 64, dtype, lens)
    P, vis, _ = decode_weights(q, k, lens, causal)
    w, out = emulate_decode_case(q, k, lens, causal, kps, dtype, natural_merge)
    return P, vis, w, out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_stays_inside_the_bound(family, dtype):
    """The rounding steps the bound is derived from, emulated: at most 0.75 of K eps P + FLOOR,
    and exact zeros at every masked key."""
    worst = {}
    P, vis, _, out = _emu_forward_case(family, dtype)
    worst["causal L384"] = readout_gate(out, P, vis, dtype, f"emulation causal {family} {IDS[dtype]}", limit=0.75)
    for causal in (False, True):
        P, vis, _, out = _emu_decode_case(family, dtype, causal)
        worst[f"decode Lk1041 causal={causal}"] = readout_gate(
            out, P, vis, dtype, f"emulation decode causal={causal} {family} {IDS[dtype]}", limit=0.75)
    # Lk = 200 in three splits, len 130: the causal tail over the split edge at 128; one split
    for (H, Hkv, Lq), ns in itertools.product(((4, 2, 3), (4, 2, 13)), (1, 3)):
        from exploring_flash_attention_amd import ops
        kps = ops.decode_plan(2, H, Hkv, Lq, 200, 64, ns, cus=256)[1]
        q, k = decode_inputs(family, 2, H, Hkv, Lq, 200, 64, dtype, (130, 5))
        P, vis, _ = decode_weights(q, k, (130, 5), True)
        _, out = emulate_decode_case(q, k, (130, 5), True, kps, dtype)
        worst[f"decode Lk200 Lq{Lq} ns{ns}"] = readout_gate(out, P, vis, dtype, f"emulation decode Lq{Lq} ns={ns}",
                                                           limit=0.75, quiet=True)
    print({k_: round(v, 3) for k_, v in worst.items()})


EMU_V2 = ((2, 64, 512, 64), (2, 64, 512, 256), (1, 128, 1000, 64), (1, 128, 1000, 256))  # H, d, L, keys per split


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("family", FAMILIES[:2])
def test_split_kv_emulation_stays_inside_the_bound(family, dtype):
    """The full (non-causal) forward, and attention_v2's steps per partial format: at most 0.75 of
    K eps P + FLOOR + split_extra -- fp32 partials under the bound as it stands."""
    worst = {}
    for H, d, L_, kps in EMU_V2:
        q, k = fwd_inputs(family, 1, H, H, L_, d, dtype)
        P, vis, s = fwd_weights(q, k, False)
        s2 = _base2(s, vis, d).reshape(H * L_, L_)
        if kps == 64:
            out = emulate_forward(s2, dtype)[1].reshape(P.shape)
            worst[f"full d{d} L{L_}"] = readout_gate(out, P, vis, dtype, "emulation full", limit=0.75, quiet=True)
        for fmt in PARTIAL_FORMATS:
            out = emulate_v2(s2, d, kps, fmt, dtype)[1].reshape(P.shape)
            r = readout_gate(out, P, vis, dtype, f"emulation v2 {fmt} d{d} L{L_} kps{kps}", limit=0.75, quiet=True,
                             extra=split_extra(P, d, kps, fmt, dtype))
            worst[fmt] = max(worst.get(fmt, 0.0), r)
    print(f"emulation {family} {IDS[dtype]}:", {k_: round(v, 3) for k_, v in worst.items()})


def _output_gate_accepts(w, P, dtype, seed):
    """The parity tests' gate (A + eps |ref|, mean_rel) on O = weights @ V, V ~ N(0, 1)."""
    d = 64
    v = torch.randn(P.shape[:-2] + (P.shape[-1], d), generator=torch.Generator().manual_seed(seed)).to(dtype)
    vn = v.double().numpy()
    out = torch.from_numpy((w.astype(np.float64) @ vn).astype(np.float32)).to(dtype)
    try:
        output_gate(out, P @ vn, dtype, "output gate", quiet=True)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_readout_gate_rejects_what_the_output_gate_accepts(dtype):
    def rejected(P, vis, out):
        leaked, bad, worst = readout_check(out, P, vis, dtype)
        return leaked > 0 or bad > 0 or worst > 1.0, (leaked, bad, round(worst, 2))

    # the clean emulation passes both gates
    P, vis, w, out = _emu_forward_case("flat", dtype)
    assert not rejected(P, vis, out)[0] and _output_gate_accepts(w, P, dtype, 1)
    P, vis, w, out = _emu_decode_case("flat", dtype)
    assert not rejected(P, vis, out)[0] and _output_gate_accepts(w, P, dtype, 2)

    # 1. the last visible key dropped in the causal rows >= 128; in row 383 alone
    P, vis, w, out = _emu_forward_case("flat", dtype, "drop")
    r, why = rejected(P, vis, out)
    assert r, why
    print("drop, rows >= 128: readout", why, "output gate accepts:", _output_gate_accepts(w, P, dtype, 1))
    P, vis, w, out = _emu_forward_case("flat", dtype, "drop", rows_from=383)
    r, why = rejected(P, vis, out)
    assert r, why
    accepts = _output_gate_accepts(w, P, dtype, 1)
    print("drop, row 383: readout", why, "output gate accepts:", accepts)
    assert accepts or dtype == torch.float16  # the gap (bf16; fp16's A = 2e-3 still sees 1.5e-3 |v|)

    # 2. the mask off by one: key i + 1 admitted
    P, vis, w, out = _emu_forward_case("flat", dtype, "admit")
    r, why = rejected(P, vis, out)
    assert r and why[0] == P.shape[0] * P.shape[1] * (EMU_FWD[3] - 1 - 128), why  # every admitted key reads nonzero
    print("admit, rows >= 128: readout", why, "output gate accepts:", _output_gate_accepts(w, P, dtype, 1))

    # 3. splits merged with e^lse although the lse are base 2: at the lengths of the GPU case (a
    # last split of 3 keys) and with whole splits only (similar lse: a few percent of weight)
    for lens in (LONG["lens"], (1024, 768)):
        P, vis, w, out = _emu_decode_case("flat", dtype, lens=lens)
        assert not rejected(P, vis, out)[0] and _output_gate_accepts(w, P, dtype, 2)
        P, vis, w, out = _emu_decode_case("flat", dtype, natural_merge=True, lens=lens)
        r, why = rejected(P, vis, out)
        assert r, why
        print(f"e^lse, lens {lens}: readout", why, "output gate accepts:", _output_gate_accepts(w, P, dtype, 2))

    # 4. the row maximum before the mask, tempt inputs: P underflows (fp16: whole rows, l = 0)
    P, vis, w, out = _emu_forward_case("tempt", dtype, "premax")
    r, why = rejected(P, vis, out)
    assert r, why
    print("premax: readout", why, "output gate accepts:", _output_gate_accepts(w, P, dtype, 1))

    # 5. a stale K tile at a chain seam: the first 64 keys of head 1's first query tile scored
    # against head 0's K (full forward, two heads); in every row of the tile, then in row 5 alone
    B, H, d, L_ = EMU_FWD
    q, k = fwd_inputs("flat", B, H, H, L_, d, dtype)
    P, vis, s = fwd_weights(q, k, False)
    stale = q[0, 1].double().numpy() @ k[0, 0, :TILE].double().numpy().T / np.sqrt(d)
    for rows in (slice(0, 128), slice(5, 6)):
        sb = s.copy()
        sb[0, 1, rows, :TILE] = stale[rows]
        w, out = emulate_forward(_base2(sb, vis, d).reshape(B * H * L_, L_), dtype)
        w, out = w.reshape(s.shape), out.reshape(s.shape)
        r, why = rejected(P, vis, out)
        assert r, (rows, why)
        print(f"stale K tile, rows {rows.start}..{rows.stop - 1}: readout", why, "output gate accepts:",
              _output_gate_accepts(w, P, dtype, 3))

    # 6. a ragged batch of 65 and 257 keys (full attention inside each sequence): the last key of
    # the longer sequence dropped in its last row alone
    for n, drop in ((65, False), (257, False), (257, True)):
        q, k = fwd_inputs("flat", 1, 1, 1, n, 64, dtype)
        P, vis, s = fwd_weights(q, k, False)
        kvis = np.array(vis)
        if drop:
            kvis[..., n - 1, n - 1] = False
        w, out = emulate_forward(_base2(s, kvis, 64).reshape(n, n), dtype)
        w, out = w.reshape(s.shape), out.reshape(s.shape)
        r, why = rejected(P, vis, out)
        assert r == drop, (n, drop, why)
        if drop:  # (the output gate's verdict is printed, not asserted)
            print("dropped last key of the 257-key sequence, row 256: readout", why, "output gate accepts:",
                  _output_gate_accepts(w, P, dtype, 4))


# ----------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CAUSAL_CASES, ids=lambda c: "B%d-H%d-d%d-L%d" % c)
def test_readout_causal_forward(gpu, case, dtype, family):
    from exploring_flash_attention_amd import ops
    B, H, d, L_ = case
    assert B * H >= _windows(L_, d)
    q, k = fwd_inputs(family, B, H, H, L_, d, dtype)
    P, vis, _ = fwd_weights(q, k, True)
    qd, kd = q.to(gpu), k.to(gpu)
    with ops.launched_kernels() as kl:
        got = read_all(lambda v: ops.attention_v1(qd, kd, v.to(gpu), causal=True), B, H, H, L_, L_, d, dtype)
    assert all("causal" in x for x in kl), kl
    readout_gate(got, P, vis, dtype, f"op=causal dtype={IDS[dtype]} family={family} d={d} L={L_}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d,L_", GQA_SHAPES, ids=[f"d{d}-L{L_}" for d, L_ in GQA_SHAPES])
def test_readout_gqa_forward(gpu, d, L_, dtype, family):
    from exploring_flash_attention_amd import ops
    worst = 0.0
    for (B, H, Hkv), causal in itertools.product(GQA_HEADS, (False, True)):
        q, k = fwd_inputs(family, B, H, Hkv, L_, d, dtype)
        P, vis, _ = fwd_weights(q, k, causal)
        qd, kd = q.to(gpu), k.to(gpu)
        with ops.launched_kernels() as kl:
            got = read_all(lambda v: ops.attention_v1(qd, kd, v.to(gpu), causal=causal), B, H, Hkv, L_, L_, d, dtype)
        assert all(", gqa>" in x and ("causal" in x) == causal for x in kl), kl
        worst = max(worst, readout_gate(got, P, vis, dtype, f"gqa B{B} H{H}/{Hkv} causal={causal}", quiet=True))
    print(f"readout op=gqa dtype={IDS[dtype]} family={family} d={d} L={L_}: worst err/bound={worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_readout_decode(gpu, d, dtype, causal, family):
    """Lk = 200: the 16-, 32- and 64-row tiles, one to three splits, the causal tail of len 130
    over the split edge at 128, sequences of 37 and 5 keys (5 < Lq: rows without a key)."""
    from exploring_flash_attention_amd import ops
    B, Lk = 2, 200
    worst = 0.0
    for (H, Hkv, Lq), lens in itertools.product(DECODE_HEADS, DECODE_LENS):
        q, k = decode_inputs(family, B, H, Hkv, Lq, Lk, d, dtype, lens)
        P, vis, _ = decode_weights(q, k, lens, causal)
        qd, kd, sl = q.to(gpu), k.to(gpu), _sl(lens, gpu)
        for ns in DECODE_SPLITS:
            got = read_all(lambda v: ops.attention_decode(qd, kd, v.to(gpu), seqlens_k=sl, causal=causal, num_splits=ns),
                           B, H, Hkv, Lq, Lk, d, dtype)
            worst = max(worst, readout_gate(got, P, vis, dtype, f"decode H{H}/{Hkv} Lq{Lq} lens={lens} ns={ns} "
                                                              f"causal={causal}", quiet=True))
    print(f"readout op=decode dtype={IDS[dtype]} family={family} d={d} Lk={Lk} causal={causal}: worst err/bound={worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("causal", (False, True), ids=("full", "causal"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
def test_readout_decode_five_splits(gpu, d, dtype, causal, family):
    """Lk = 1041 in five splits of 256 keys, len 1027 at Lq = 8: the tail keys 1020..1026 straddle
    the split edge at 1024; len 37: four splits without a key.  All 17 (d = 64) windows."""
    from exploring_flash_attention_amd import ops
    c = LONG
    B, H, Hkv, Lq, Lk, ns, lens = (c[x] for x in ("B", "H", "Hkv", "Lq", "Lk", "ns", "lens"))
    assert ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, dtype)[:2] == (5, 256)
    assert _windows(Lk, 64) == 17
    q, k = decode_inputs(family, B, H, Hkv, Lq, Lk, d, dtype, lens)
    P, vis, _ = decode_weights(q, k, lens, causal)
    qd, kd, sl = q.to(gpu), k.to(gpu), _sl(lens, gpu)
    with ops.launched_kernels() as kl:
        got = read_all(lambda v: ops.attention_decode(qd, kd, v.to(gpu), seqlens_k=sl, causal=causal, num_splits=ns),
                       B, H, Hkv, Lq, Lk, d, dtype)
    assert all("fa_decode_combine_kernel" in x for x in kl), kl
    readout_gate(got, P, vis, dtype, f"op=decode dtype={IDS[dtype]} family={family} d={d} Lk={Lk} causal={causal}")


def _scatter(x, table, ps, nblk):
    """Pool [nblk, ps, H_kv, d] holding x [B, H_kv, Lk, d] under `table` [B, P]; NaN in every row
    no key lives in (unreferenced blocks, the rest of a last page)."""
    B, Hkv, Lk, d = x.shape
    pool = torch.full((nblk, ps, Hkv, d), float("nan"), dtype=x.dtype)
    for b in range(B):
        for p in range(-(-Lk // ps)):
            rows = min(ps, Lk - p * ps)
            pool[table[b, p], :rows] = x[b, :, p * ps:p * ps + rows].transpose(0, 1)
    return pool


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("ps", PAGES)
def test_readout_paged_decode(gpu, ps, d, dtype, family):
    """The five-split case through a shuffled block table: the readout gate, and bit for bit the
    contiguous call on the gathered cache."""
    from exploring_flash_attention_amd import ops
    c = LONG
    B, H, Hkv, Lq, Lk, ns, lens = (c[x] for x in ("B", "H", "Hkv", "Lq", "Lk", "ns", "lens"))
    assert ops.decode_plan(B, H, Hkv, Lq, Lk, d, ns, dtype)[:2] == (5, 256)
    npages = -(-Lk // ps)
    nblk = B * npages + 5
    table = torch.tensor(_perm_table(B, npages, nblk, seed=ps + d), dtype=torch.int32).reshape(B, npages)
    assert not torch.equal(table.reshape(-1), torch.arange(B * npages, dtype=torch.int32))  # shuffled
    q, k = decode_inputs(family, B, H, Hkv, Lq, Lk, d, dtype, lens)
    qd, kd, sl, td = q.to(gpu), k.to(gpu), _sl(lens, gpu), table.to(gpu)
    kp = _scatter(k, table, ps, nblk).to(gpu)
    worst = 0.0
    for causal in (False, True):
        P, vis, _ = decode_weights(q, k, lens, causal)

        def call(v):
            got = ops.attention_decode_paged(qd, kp, _scatter(v, table, ps, nblk).to(gpu), td, seqlens_k=sl,
                                             max_seqlen_k=Lk, causal=causal, num_splits=ns)
            want = ops.attention_decode(qd, kd, v.to(gpu), seqlens_k=sl, causal=causal, num_splits=ns)
            assert torch.equal(_bits(got), _bits(want)), (ps, d, causal)
            return got

        with ops.launched_kernels() as kl:
            got = read_all(call, B, H, Hkv, Lq, Lk, d, dtype)
        assert sum(", paged>" in x for x in kl) == len(kl) // 2, kl
        worst = max(worst, readout_gate(got, P, vis, dtype, f"paged ps{ps} causal={causal}", quiet=True))
    print(f"readout op=paged dtype={IDS[dtype]} family={family} d={d} ps={ps}: worst err/bound={worst:.3f}")
