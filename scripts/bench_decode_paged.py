#!/usr/bin/env python3
"""Paged KV-cache decode (ops.attention_decode_paged) at d = 128 bf16 against the contiguous
decode and against the gather a caller without it needs, timed with bench.py's own method (its
time_step / clock_settle / launched helpers), all forms in ONE process on one device, alternating
windows, the median of --rounds windows reported.

    python scripts/bench_decode_paged.py [--steps 500 --warmup 300 --rounds 3 --out profiles/decode_paged_bench.json]

Shapes: those of scripts/bench_decode.py (H32 H_kv8 Lk8192, B in {1, 16, 64} at Lq = 1, B16 at
Lq = 4 causal).  Per shape:
  (a)    attention_decode(q, k, v)                    k, v [B, H_kv, Lk, d] contiguous
  (p64), (p128), (p256)
         attention_decode_paged(q, kp, vp, table)     a [num_blocks, page_size, H_kv, d] pool of
                                                      the same total size, the pages of the
                                                      sequences shuffled over it
  (s)    attention_decode on a [B, Lk, H_kv, d] cache passed transposed: the contiguous form at
         the pool's row stride (H_kv * d), which separates the layout's share of (p) - (a) from
         the table's
  (h128) attention_decode_paged on a [num_blocks, H_kv, 128, d] pool passed transposed (a
         page's rows of one head contiguous, as in (a))
  (g)    index_select of every sequence's pages (page size 128) into a contiguous
         [B, Lk, H_kv, d] cache, then (a) on it read in place: what a paged caller does today
out and workspace are given everywhere.  (p) moves the bytes of (a) plus 4 bytes per 64-key tile,
so (p) / (a) beyond the spread of the windows is the cost of the address chain (table entry ->
descriptor -> loads).  Acceptance: (p) beats (g) by more than the spread at every shape and page
size.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (B, H, H_kv, Lq, Lk, d, causal)
SHAPES = ((1, 32, 8, 1, 8192, 128, False), (16, 32, 8, 1, 8192, 128, False), (64, 32, 8, 1, 8192, 128, False),
          (16, 32, 8, 4, 8192, 128, True))
PAGES = (64, 128, 256)
GATHER_PAGE = 128


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows of every form; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_paged_bench.json"))
    ap.add_argument("--note", default=None, help="free text recorded in the result (e.g. the kernel variant)")
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_decode_paged.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), all forms alternating in one process",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16", "note": args.note,
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "cases": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    gen = torch.Generator().manual_seed(99)
    for B, H, Hkv, Lq, Lk, d, causal in SHAPES:
        q, _, _ = bench._make_inputs(torch, dev, B, H, Lq, d, seed=1234)
        _, k, v = bench._make_inputs(torch, dev, B, Hkv, 1, d, seed=4321, Lk=Lk)
        out = torch.empty_like(q)
        splits, kps, nbytes = ops.decode_plan(B, H, Hkv, Lq, Lk, d)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        steps = {"a": lambda: ops.attention_decode(q, k, v, causal=causal, out=out, workspace=ws)}
        want = ops.attention_decode(q, k, v, causal=causal).clone()
        pools, bitwise = {}, {}
        for ps in PAGES:
            P = Lk // ps
            perm = torch.randperm(B * P, generator=gen)
            table = perm.reshape(B, P).to(torch.int32).to(dev)
            kp, vp = (torch.empty((B * P, ps, Hkv, d), dtype=q.dtype, device=dev) for _ in range(2))
            # page p of sequence b goes to block table[b, p]: the pool holds the cache of (a)
            kp[perm.to(dev)] = k.transpose(1, 2).reshape(B * P, ps, Hkv, d)
            vp[perm.to(dev)] = v.transpose(1, 2).reshape(B * P, ps, Hkv, d)
            pools[ps] = (kp, vp, table)
            steps[f"p{ps}"] = (lambda kp=kp, vp=vp, table=table: ops.attention_decode_paged(
                q, kp, vp, table, max_seqlen_k=Lk, causal=causal, out=out, workspace=ws))
            got = ops.attention_decode_paged(q, kp, vp, table, max_seqlen_k=Lk, causal=causal)
            bitwise[ps] = bool(torch.equal(got.view(torch.int16), want.view(torch.int16)))
        ks, vs = k.transpose(1, 2).contiguous().transpose(1, 2), v.transpose(1, 2).contiguous().transpose(1, 2)
        steps["s"] = lambda: ops.attention_decode(q, ks, vs, causal=causal, out=out, workspace=ws)
        kp, vp, table = pools[128]
        kh, vh = kp.transpose(1, 2).contiguous().transpose(1, 2), vp.transpose(1, 2).contiguous().transpose(1, 2)
        steps["h128"] = (lambda kh=kh, vh=vh, table=table: ops.attention_decode_paged(
            q, kh, vh, table, max_seqlen_k=Lk, causal=causal, out=out, workspace=ws))
        kp, vp, table = pools[GATHER_PAGE]
        idx = table.reshape(-1).long()
        kg, vg = torch.empty_like(kp), torch.empty_like(vp)

        def gather_then_decode():
            torch.index_select(kp, 0, idx, out=kg)
            torch.index_select(vp, 0, idx, out=vg)
            return ops.attention_decode(q, kg.view(B, Lk, Hkv, d).transpose(1, 2), vg.view(B, Lk, Hkv, d).transpose(1, 2),
                                        causal=causal, out=out, workspace=ws)

        steps["g"] = gather_then_decode
        g_bitwise = bool(torch.equal(gather_then_decode().view(torch.int16), want.view(torch.int16)))
        labels = {n: bench.launched(ops, steps[n]) for n in steps}
        bench.clock_settle(torch, steps["a"], 0.25)
        order = list(steps)
        times = {n: [] for n in order}
        for _ in range(args.rounds):
            for n in order:
                times[n].append(ms(steps[n]))
        med = {n: statistics.median(t) for n, t in times.items()}
        spread = max(max(t) - min(t) for t in times.values())
        read_bytes = (q.numel() + k.numel() + v.numel()) * 2
        rec = {"B": B, "H": H, "H_kv": Hkv, "Lq": Lq, "Lk": Lk, "d": d, "causal": causal,
               "splits": splits, "keys_per_split": kps,
               "a_decode_ms": round(med["a"], 5),
               "p_paged_ms": {str(ps): round(med[f"p{ps}"], 5) for ps in PAGES},
               "s_decode_row_strided_ms": round(med["s"], 5), "h128_paged_head_major_ms": round(med["h128"], 5),
               "s_over_a": round(med["s"] / med["a"], 4), "h128_over_a": round(med["h128"] / med["a"], 4),
               "p_over_s": {str(ps): round(med[f"p{ps}"] / med["s"], 4) for ps in PAGES},
               "g_gather_then_decode_ms": round(med["g"], 5), "gather_page_size": GATHER_PAGE,
               "windows_ms": {n: [round(x, 5) for x in t] for n, t in times.items()},
               "window_spread_ms": round(spread, 5),
               "p_over_a": {str(ps): round(med[f"p{ps}"] / med["a"], 4) for ps in PAGES},
               "p_minus_a_over_spread": {str(ps): round((med[f"p{ps}"] - med["a"]) / spread, 2) if spread > 0 else None
                                         for ps in PAGES},
               "p_beats_g": {str(ps): bool(med["g"] - med[f"p{ps}"] > spread) for ps in PAGES},
               "g_over_p": {str(ps): round(med["g"] / med[f"p{ps}"], 3) for ps in PAGES},
               "bytes_read": read_bytes,
               "a_read_GBps": round(read_bytes / (med["a"] * 1e-3) / 1e9, 1),
               "p_read_GBps": {str(ps): round(read_bytes / (med[f"p{ps}"] * 1e-3) / 1e9, 1) for ps in PAGES},
               "paged_bitwise_equal_to_a": {str(ps): bitwise[ps] for ps in PAGES}, "gather_bitwise_equal_to_a": g_bitwise,
               "a_kernel": labels["a"], "p_kernel": labels[f"p{PAGES[0]}"]}
        result["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        write()
        del q, k, v, out, ws, steps, pools, kp, vp, kg, vg, ks, vs, kh, vh, table, idx, want
        torch.cuda.empty_cache()

    bad = [(r["B"], r["Lq"], ps) for r in result["cases"] for ps, ok in r["p_beats_g"].items() if not ok]
    bad += [(r["B"], r["Lq"], ps) for r in result["cases"] for ps, ok in r["paged_bitwise_equal_to_a"].items() if not ok]
    if bad:
        print("attention_decode_paged does not beat the gather (or differs from attention_decode) at", bad, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
