#!/usr/bin/env python3
"""The grouped MoE expert FFN forward (moe_expert_up + moe_expert_gemm, the
moe_nn kernels of csrc/gemm_kernels.hip) against the chain it replaces:
bmm, bmm, silu * mul, bmm on hipBLASLt and aten.  Forward only, bf16.

Shapes: the Mixtral per-GPU shape (E 8, d 4096, ffn 14336, cap from
capacity(N, 8, 2, 1.25) for --tokens tokens) and MIXTRAL_SMALL's.  Routing:
balanced (every expert's capacity 80% full, what capacity_factor 1.25 leaves
when no expert overflows) and skewed (half the experts empty, the others
full).  The chain multiplies every slot whatever the routing; the grouped
path is timed with `valid` (empty 128-row tiles skipped) and, on the balanced
routing, without.

Times are torch.cuda.Event windows around --iters back-to-back calls, after
a warm-up of every configuration, the configurations alternating inside each
of --repeats repeats; median [min-max] over the repeats.  TFLOP/s counts the
dense 6 E cap d ffn flops for every configuration.  One JSON line per
configuration, then one summary line per shape.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F

import easydist_amd.ops as ops
from easydist_amd.ops import moe_ffn as mf
from easydist_amd.ops.moe_ops import capacity

# name -> (tokens or None for --tokens, E, d, ffn)
SHAPES = {"mixtral": (None, 8, 4096, 14336), "mixtral_small": (512, 4, 256, 512)}


def event_us(fn, iters):
    """Device us per call over one event window of `iters` calls."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def bench_shape(name, shape, args):
    tokens, E, d, ffn = shape
    tokens = tokens or args.tokens
    cap = capacity(tokens, E, 2, 1.25)
    torch.manual_seed(0)
    bf = torch.bfloat16
    w1, w3 = (torch.randn(E, d, ffn, device="cuda").to(bf) * d ** -0.5
              for _ in range(2))
    w2 = torch.randn(E, ffn, d, device="cuda").to(bf) * ffn ** -0.5
    rows = torch.arange(cap, device="cuda").expand(E, cap)
    counts = {"balanced": torch.full((E, 1), int(cap / 1.25)),
              "skewed": (torch.arange(E) % 2 * cap).unsqueeze(1)}
    cfgs = {}
    for routing, cnt in counts.items():
        valid = rows < cnt.cuda()
        x = torch.randn(E, cap, d, device="cuda").to(bf) * valid.unsqueeze(-1)
        assert mf._kernel_ok(x, valid, w1, w3)

        def chain(x=x):
            a = torch.bmm(x, w1)
            b = torch.bmm(x, w3)
            return torch.bmm(F.silu(a) * b, w2)

        def grouped(x=x, valid=valid):
            h, _, _ = mf.moe_expert_up(x, w1, w3, valid)
            return mf.moe_expert_gemm(h, w2, valid)

        cfgs[routing, "chain"] = chain
        cfgs[routing, "grouped"] = grouped
        if routing == "balanced":
            cfgs[routing, "grouped_no_valid"] = \
                lambda x=x: grouped(x, None)
    for fn in cfgs.values():
        for _ in range(args.warm_iters):
            fn()
    torch.cuda.synchronize()
    times = {c: [] for c in cfgs}
    for _ in range(args.repeats):
        for c, fn in cfgs.items():   # alternate configs inside a repeat
            times[c].append(event_us(fn, args.iters))

    flops = 6 * E * cap * d * ffn
    summary = {"shape": name}
    for (routing, cfg), xs in times.items():
        med = statistics.median(xs)
        print(json.dumps({
            "shape": name, "dims": {"E": E, "cap": cap, "d": d, "ffn": ffn},
            "routing": routing, "config": cfg,
            "us": {"med": round(med, 1), "min": round(min(xs), 1),
                   "max": round(max(xs), 1)},
            "dense_tflops": round(flops / med / 1e6, 1)}), flush=True)
        summary[f"{routing}_{cfg}_us"] = round(med, 1)
    for routing in counts:
        summary[f"{routing}_chain_over_grouped_time"] = round(
            summary[f"{routing}_chain_us"] / summary[f"{routing}_grouped_us"],
            2)
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8192,
                    help="tokens per GPU of the mixtral shape")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm-iters", type=int, default=3)
    args = ap.parse_args()

    assert ops.load_extension() is not None and torch.cuda.is_available(), \
        "bench_moe_experts needs the HIP extension and a GPU"
    for name in args.shapes.split(","):
        bench_shape(name, SHAPES[name], args)


if __name__ == "__main__":
    main()
