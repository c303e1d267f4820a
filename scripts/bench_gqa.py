#!/usr/bin/env python3
"""Grouped-query attention_v1 against the MHA call on pre-expanded K / V at d = 128 bf16, timed
with bench.py's own method (its time_step / clock_settle / launched helpers, the same --steps /
--warmup defaults), all forms in ONE process on one device, alternating windows.

    python scripts/bench_gqa.py [--steps 500 --warmup 300 --rounds 3 --out profiles/gqa_bench.json]

Per shape (B4 H32 H_kv8 L4096, B32 H8 H_kv2 L1024), causal and non-causal:
  (a) attention_v1(q, k, v)                      k, v [B, H_kv, L, d]: the GQA kernels
  (b) attention_v1(q, k_exp, v_exp)              k, v expanded to H heads beforehand (not timed)
  (c) the expansion alone                        k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
Acceptance: (a) is not slower than (b) by more than the spread of the run's windows.  Both
numbers are written down whatever they are.  Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((4, 32, 8, 4096, 128), (32, 8, 2, 1024, 128))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3, help="alternating (a), (b), (c) windows; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gqa_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_gqa.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), (a), (b), (c) alternating in one process",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
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

    for B, H, Hkv, L, d in SHAPES:
        G = H // Hkv
        q, _, _ = bench._make_inputs(torch, dev, B, H, L, d, seed=1234)
        _, k, v = bench._make_inputs(torch, dev, B, Hkv, L, d, seed=4321)
        ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        out = torch.empty_like(q)
        for causal in (False, True):
            steps = {"a": lambda: ops.attention_v1(q, k, v, out=out, causal=causal),
                     "b": lambda: ops.attention_v1(q, ke, ve, out=out, causal=causal),
                     "c": lambda: (k.repeat_interleave(G, 1), v.repeat_interleave(G, 1))}
            labels = {n: bench.launched(ops, steps[n]) for n in ("a", "b")}
            oa = ops.attention_v1(q, k, v, causal=causal)
            ob = ops.attention_v1(q, ke, ve, causal=causal)
            bitwise = bool(torch.equal(oa, ob))
            del oa, ob
            bench.clock_settle(torch, steps["b"], 0.25)
            times = {n: [] for n in steps}
            for _ in range(args.rounds):
                for n in steps:
                    times[n].append(ms(steps[n]))
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = max(max(t) - min(t) for n, t in times.items() if n != "c")
            nqt = (L + 127) // 128
            work = bench.flops(B, H, L, d) * ((nqt + 1) / (2 * nqt) if causal else 1.0)
            rec = {"B": B, "H": H, "H_kv": Hkv, "L": L, "d": d, "causal": causal, "bitwise_equal": bitwise,
                   "a_gqa_ms": round(med["a"], 5), "b_mha_expanded_ms": round(med["b"], 5),
                   "c_expand_copy_ms": round(med["c"], 5),
                   "a_windows_ms": [round(x, 5) for x in times["a"]], "b_windows_ms": [round(x, 5) for x in times["b"]],
                   "c_windows_ms": [round(x, 5) for x in times["c"]],
                   "window_spread_ms": round(spread, 5), "a_minus_b_ms": round(med["a"] - med["b"], 5),
                   "a_not_slower_than_b": bool(med["a"] - med["b"] <= spread),
                   "a_kernel": labels["a"], "b_kernel": labels["b"],
                   "a_tflops": round(work / (med["a"] * 1e-3) / 1e12, 1),
                   "b_tflops": round(work / (med["b"] * 1e-3) / 1e12, 1),
                   "algorithmic_bytes_a": (2 * B * H + 2 * B * Hkv) * L * d * 2,
                   "algorithmic_bytes_b": 4 * B * H * L * d * 2}
            result["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            write()
        del q, k, v, ke, ve, out, steps
        torch.cuda.empty_cache()

    bad = [r for r in result["cases"] if not (r["a_not_slower_than_b"] and r["bitwise_equal"])]
    if bad:
        print("GQA slower than MHA on expanded K/V (or not bitwise equal) at",
              [(r["B"], r["H"], r["H_kv"], r["L"], r["causal"]) for r in bad], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
