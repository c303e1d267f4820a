#!/usr/bin/env python3
"""attention_varlen with key lengths of their own (cu_seqlens_k / seqused_k: chunked prefill against
a prefix) against what the library offered before it, at d = 128 bf16, H32 H_kv8, causal, timed
with bench.py's own method (time_step / clock_settle / launched), all forms in ONE process on one
device, alternating windows, median of the rounds.

    python scripts/bench_varlen_kv.py [--steps 20 --warmup 5 --rounds 3 --out profiles/varlen_kv_bench.json]

Cases:
  (a) 16 sequences, 512 new tokens each against 8192 keys (a prefix of 7680 and the chunk itself):
        new        attention_varlen(q_chunk, k, v, cu_q, 512, causal=True, cu_seqlens_k=, max_seqlen_k=8192)
        recompute  attention_varlen(causal=True) on all 8192 queries of every sequence -- the only
                   exact form the library had
        sdpa       torch scaled_dot_product_attention with an explicit [512, 8192] boolean mask, K / V
                   expanded to H heads beforehand (an error is recorded, not hidden)
  (b) the same 16 x 8192 prefill as 16 chunks of 512 through the new call (seqused_k grows by 512 per
      chunk on the k / v tensors read in place), the 16 calls summed, against the one-shot call
  (c) cu_seqlens_k = cu_seqlens on 16 x 4096 (scripts/bench_varlen.py's batch i) against the
      self-attention call on the same batch
Also recorded: the 128-row x 64-key tiles each form walks, and whether the new call's rows equal the
one-shot call's bit for bit.  No ratio is fixed in advance.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV, D = 32, 8, 128
BQ, BK = 128, 64


def kv_tiles(len_q, len_k):
    """KV tiles one head of a causal (len_q, len_k) sequence walks: per query tile, the keys up to
    the diagonal of its last row."""
    s = len_k - len_q
    return sum((min(max(s + BQ * (qt + 1), 0), len_k) + BK - 1) // BK for qt in range((len_q + BQ - 1) // BQ))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows of every form; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_kv_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_varlen_kv.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), the forms alternating in one process, "
                        "median of --rounds windows; window_spread_ms = the largest max - min over a form's windows",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
              "H": H, "H_kv": HKV, "d": D, "causal": True,
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "cases": []}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    def measure(steps, settle):
        bench.clock_settle(torch, settle, 0.25)
        times = {n: [] for n in steps}
        for _ in range(args.rounds):
            for n in steps:
                times[n].append(ms(steps[n]))
        med = {n: statistics.median(t) for n, t in times.items()}
        return med, times, max(max(t) - min(t) for t in times.values())

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, dtype=torch.bfloat16, generator=g)

    def tflops(tiles, t_ms):
        return round(4.0 * tiles * BQ * BK * D / (t_ms * 1e-3) / 1e12, 1)

    g = torch.Generator(device=dev).manual_seed(1234)

    # ---- (a) and (b): 16 sequences of 8192 tokens, chunks of 512
    B, L, C = 16, 8192, 512
    NC = L // C
    q, k, v = rnd(B * L, H, D), rnd(B * L, HKV, D), rnd(B * L, HKV, D)
    cu_full = i32([b * L for b in range(B + 1)])
    cu_chunk = i32([b * C for b in range(B + 1)])
    out_full = torch.empty_like(q)
    # chunk c of every sequence as a packed [B * C, H, d] tensor, made beforehand
    q_chunks = [q.view(B, L, H, D)[:, c * C:(c + 1) * C].reshape(B * C, H, D).contiguous() for c in range(NC)]
    out_chunks = [torch.empty_like(t) for t in q_chunks]
    used = [i32([(c + 1) * C] * B) for c in range(NC)]

    def one_shot():
        ops.attention_varlen(q, k, v, cu_full, L, causal=True, out=out_full)

    def chunk(c):
        ops.attention_varlen(q_chunks[c], k, v, cu_chunk, C, causal=True, out=out_chunks[c], cu_seqlens_k=cu_full,
                             max_seqlen_k=L, seqused_k=used[c])

    def last_chunk():
        chunk(NC - 1)

    def all_chunks():
        for c in range(NC):
            chunk(c)

    ke, ve = (t.view(B, L, HKV, D).transpose(1, 2).repeat_interleave(H // HKV, 1) for t in (k, v))
    q_last = q_chunks[NC - 1].view(B, C, H, D).transpose(1, 2)
    mask = (torch.arange(L, device=dev)[None, :] <= torch.arange(C, device=dev)[:, None] + (L - C))

    def sdpa():
        torch.nn.functional.scaled_dot_product_attention(q_last, ke, ve, attn_mask=mask)

    steps_a = {"new": last_chunk, "recompute": one_shot, "sdpa": sdpa}
    sdpa_error = None
    try:
        sdpa()
        torch.cuda.synchronize()
    except Exception as e:  # recorded below
        sdpa_error = f"{type(e).__name__}: {str(e)[:200]}"
        del steps_a["sdpa"]
    labels = {"new": bench.launched(ops, last_chunk), "recompute": bench.launched(ops, one_shot)}
    one_shot()
    all_chunks()
    torch.cuda.synchronize()
    want = out_full.view(B, L, H, D)
    same = all(torch.equal(out_chunks[c].view(B, C, H, D), want[:, c * C:(c + 1) * C]) for c in range(NC))
    tiles_new = B * H * kv_tiles(C, L)
    tiles_full = B * H * kv_tiles(L, L)
    med, times, spread = measure(steps_a, one_shot)
    rec = {"case": "a", "what": "16 sequences, 512 new tokens each against 8192 keys", "B": B, "len_q": C, "len_k": L,
           "new_ms": round(med["new"], 5), "recompute_all_queries_ms": round(med["recompute"], 5),
           "torch_sdpa_masked_ms": round(med["sdpa"], 5) if "sdpa" in med else None, "sdpa_error": sdpa_error,
           "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()}, "window_spread_ms": round(spread, 5),
           "recompute_over_new": round(med["recompute"] / med["new"], 3),
           "sdpa_over_new": round(med["sdpa"] / med["new"], 3) if "sdpa" in med else None,
           "kv_tiles_new": tiles_new, "kv_tiles_recompute": tiles_full,
           "new_us_per_kilotile": round(med["new"] * 1e6 / tiles_new, 3),
           "recompute_us_per_kilotile": round(med["recompute"] * 1e6 / tiles_full, 3),
           "new_tflops": tflops(tiles_new, med["new"]), "recompute_tflops": tflops(tiles_full, med["recompute"]),
           "new_kernel": labels["new"], "recompute_kernel": labels["recompute"],
           "chunk_rows_equal_one_shot_bitwise": bool(same)}
    result["cases"].append(rec)
    print(json.dumps(rec), flush=True)
    write()

    med, times, spread = measure({"chunked": all_chunks, "one_shot": one_shot}, one_shot)
    tiles_chunked = B * H * sum(kv_tiles(C, (c + 1) * C) for c in range(NC))
    rec = {"case": "b", "what": "16 x 8192 prefill as 16 chunks of 512 (16 calls summed) against the one-shot call",
           "B": B, "chunks": NC, "chunk": C, "chunked_ms": round(med["chunked"], 5),
           "one_shot_ms": round(med["one_shot"], 5), "chunked_over_one_shot": round(med["chunked"] / med["one_shot"], 4),
           "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()}, "window_spread_ms": round(spread, 5),
           "kv_tiles_chunked": tiles_chunked, "kv_tiles_one_shot": tiles_full,
           "chunked_us_per_kilotile": round(med["chunked"] * 1e6 / tiles_chunked, 3),
           "one_shot_us_per_kilotile": round(med["one_shot"] * 1e6 / tiles_full, 3),
           "chunked_tflops": tflops(tiles_chunked, med["chunked"]), "one_shot_tflops": tflops(tiles_full, med["one_shot"]),
           "chunk_rows_equal_one_shot_bitwise": bool(same)}
    result["cases"].append(rec)
    print(json.dumps(rec), flush=True)
    write()
    del q, k, v, out_full, q_chunks, out_chunks, ke, ve, q_last, mask
    torch.cuda.empty_cache()

    # ---- (c): the same lengths on both sides, 16 x 4096
    B, L = 16, 4096
    q, k, v = rnd(B * L, H, D), rnd(B * L, HKV, D), rnd(B * L, HKV, D)
    cu = i32([b * L for b in range(B + 1)])
    cu_k = cu.clone()
    out_self, out_kv = torch.empty_like(q), torch.empty_like(q)

    def self_attn():
        ops.attention_varlen(q, k, v, cu, L, causal=True, out=out_self)

    def kv_form():
        ops.attention_varlen(q, k, v, cu, L, causal=True, out=out_kv, cu_seqlens_k=cu_k, max_seqlen_k=L)

    labels = {"self": bench.launched(ops, self_attn), "kv": bench.launched(ops, kv_form)}
    torch.cuda.synchronize()
    same = torch.equal(out_self, out_kv)
    med, times, spread = measure({"kv": kv_form, "self": self_attn}, self_attn)
    tiles = B * H * kv_tiles(L, L)
    rec = {"case": "c", "what": "cu_seqlens_k = cu_seqlens on 16 x 4096 against the self-attention call", "B": B,
           "L": L, "kv_form_ms": round(med["kv"], 5), "self_attention_ms": round(med["self"], 5),
           "kv_over_self": round(med["kv"] / med["self"], 4),
           "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()}, "window_spread_ms": round(spread, 5),
           "spread_over_self": round(spread / med["self"], 4), "kv_tiles": tiles,
           "kv_form_tflops": tflops(tiles, med["kv"]), "self_attention_tflops": tflops(tiles, med["self"]),
           "kv_kernel": labels["kv"], "self_kernel": labels["self"], "bitwise_equal": bool(same)}
    result["cases"].append(rec)
    print(json.dumps(rec), flush=True)
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
