#!/usr/bin/env python3
"""Causal against non-causal attention_v1 at d = 128 bf16, timed with bench.py's own method
(its time_step / clock_settle / launched helpers, the same --steps / --warmup defaults), both
forms in ONE process on one device, alternating, so that the ratio does not depend on the box.

    python scripts/bench_causal.py [--steps 500 --warmup 300 --rounds 3 --out profiles/causal_bench.json]

Per shape (B32 H8 L1024 = C3, B32 H8 L4096):
  (a) attention_v1(causal=True)    fa_fwd_kernel<final, causal>, the 32x32x16 kernel
  (b) attention_v1(causal=False)   as shipped: the d = 128 chain kernel
  (c) the non-causal 32x32x16 fa_fwd_kernel at d = 128 is not reachable through the library for
      these shapes (whole 64-key tiles always take the 16x16x32 kernels), so it is left out.
The ideal ratio (a)/(b) by MFMA work is (nqt + 1) / (2 nqt) in 128-row query tiles.
torch's scaled_dot_product_attention(is_causal=True) is timed last as context where it runs.
Needs a ROCm GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((32, 8, 1024, 128), (32, 8, 4096, 128))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3, help="alternating (a), (b) windows per shape; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "causal_bench.json"))
    ap.add_argument("--no-sdpa", action="store_true")
    args = ap.parse_args(argv)

    import torch

    import bench
    from exploring_flash_attention_amd import ops

    assert torch.cuda.is_available(), "bench_causal.py needs a ROCm GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    props = torch.cuda.get_device_properties(dev)
    result = {"method": "bench.py time_step (device events around --steps back-to-back calls after --warmup "
                        "untimed ones and a 0.25 s clock settle), (a) and (b) alternating in one process",
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "dtype": "bf16",
              # (boxes differ by a few per cent in sustained clock: (b) at L = 1024 is bench.py's C3 and
              # places this one in the range DESIGN.md records)
              "box": {"device": props.name, "compute_units": props.multi_processor_count,
                      "torch": torch.__version__, "hip": torch.version.hip},
              "c_noncausal_32x32x16": "left out: not reachable through the library at these shapes",
              "shapes": []}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    def ms(step):
        _, ev = bench.time_step(torch, step, args.steps, args.warmup, lambda: None)
        return ev / args.steps

    for B, H, L, d in SHAPES:
        q, k, v = bench._make_inputs(torch, dev, B, H, L, d, seed=1234)
        out = torch.empty_like(q)
        steps = {"a": lambda: ops.attention_v1(q, k, v, out=out, causal=True),
                 "b": lambda: ops.attention_v1(q, k, v, out=out)}
        labels = {n: bench.launched(ops, s) for n, s in steps.items()}
        bench.clock_settle(torch, steps["b"], 0.25)
        times = {"a": [], "b": []}
        for _ in range(args.rounds):
            for n in ("a", "b"):
                times[n].append(ms(steps[n]))
        a_ms, b_ms = (statistics.median(times[n]) for n in ("a", "b"))
        nqt = (L + 127) // 128
        rec = {"B": B, "H": H, "L": L, "d": d,
               "a_causal_ms": round(a_ms, 5), "b_noncausal_ms": round(b_ms, 5), "c_noncausal_32x32x16_ms": None,
               "a_windows_ms": [round(x, 5) for x in times["a"]], "b_windows_ms": [round(x, 5) for x in times["b"]],
               "ratio_a_over_b": round(a_ms / b_ms, 4), "ideal_work_ratio": round((nqt + 1) / (2 * nqt), 4),
               "a_kernel": labels["a"], "b_kernel": labels["b"],
               "a_tflops_of_causal_work": round(bench.flops(B, H, L, d) * (nqt + 1) / (2 * nqt) / (a_ms * 1e-3) / 1e12, 1),
               "b_tflops": round(bench.flops(B, H, L, d) / (b_ms * 1e-3) / 1e12, 1)}
        result["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
        write()
        del q, k, v, out, steps
        torch.cuda.empty_cache()

    if not args.no_sdpa:  # context only, never a gate
        for rec in result["shapes"]:
            try:
                q, k, v = bench._make_inputs(torch, dev, rec["B"], rec["H"], rec["L"], rec["d"], seed=1234)
                sd = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)  # noqa: E731
                _, ev = bench.time_step(torch, sd, 50, 20, lambda: None)
                rec["torch_sdpa_is_causal_ms"] = round(ev / 50, 5)
                del q, k, v
            except Exception as exc:  # noqa: BLE001 -- context: reported, not fatal
                rec["torch_sdpa_is_causal_ms"] = None
                rec["torch_sdpa_error"] = f"{type(exc).__name__}: {exc}"[:200]
            print(json.dumps({"L": rec["L"], "torch_sdpa_is_causal_ms": rec["torch_sdpa_is_causal_ms"]}), flush=True)
            write()
            torch.cuda.empty_cache()
    bad = [r for r in result["shapes"] if not r["a_causal_ms"] < r["b_noncausal_ms"]]
    if bad:
        print("causal is not faster than non-causal at", [(r["B"], r["H"], r["L"]) for r in bad], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
