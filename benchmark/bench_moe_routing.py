#!/usr/bin/env python3
"""The MoE routing kernels (csrc/moe_kernels.hip) against the aten path they
replace and against a device-to-device copy of the bytes each op must move.

Ops, on bf16 [N, C] token rows and [E, cap, C] bins (T = 2 N K C bytes, the
rows that routing keeps when nothing is dropped; B = 2 E cap C bytes):

  moe_bins         reads T, writes B            (empty slots are written too)
  moe_combine      reads T, writes T / K
  moe_bins_bwd     reads T, writes T / K
  moe_combine_bwd  reads 2 T, writes B

Each op is timed through torch.ops.easydist_amd with the kernels, again with
EASYDIST_MOE_HIP=0 (the aten path) and as a copy of half the bytes above (a
copy reads and writes each byte).  Shape: MIXTRAL_SMALL's (N 512, C 256,
E 4, K 2), or one given on the command line; only shapes inside the kernels'
envelope (C <= 512) are timed, anything else is an error.  At this size a
call is a few launches of a few microseconds each, so the times are
launch-bound: they compare launch counts more than bandwidth.

Times are torch.cuda.Event windows around --iters back-to-back calls, after
a warm-up of every configuration, the configurations alternating inside each
of --repeats repeats; median [min-max] over the repeats.  TB/s is the op's
bytes over the median time, whatever the configuration really moves.  One
JSON line per op and configuration, then one summary line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import easydist_amd.ops as ops
from easydist_amd.ops import moe_ops as mo

# name -> (N, C, E, K, factor)
SHAPES = {"mixtral_small": (512, 256, 4, 2, 1.25)}
OPS = ("moe_bins", "moe_combine", "moe_bins_bwd", "moe_combine_bwd")


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


def aten(fn):
    def run():
        os.environ["EASYDIST_MOE_HIP"] = "0"
        try:
            return fn()
        finally:
            os.environ.pop("EASYDIST_MOE_HIP")
    return run


def bench_shape(name, shape, args):
    N, C, E, K, factor = shape
    torch.manual_seed(0)
    bf = torch.bfloat16
    tokens = torch.randn(N, C, device="cuda").to(bf)
    probs = torch.softmax(torch.randn(N, E, device="cuda"), -1)
    topv, topi = probs.topk(K, dim=-1)
    topv = (topv / topv.sum(-1, keepdim=True)).to(bf)
    ed = torch.ops.easydist_amd
    assert mo._bins_kernel_ok(tokens, topi, topv, E, factor), \
        "shape outside the kernels' envelope"
    bins, gates, src, valid = ed.moe_bins(tokens, topi, topv, E, factor)
    cap = bins.shape[1]
    xbins = torch.randn_like(bins)
    gbins = torch.randn_like(bins)
    ggates = torch.randn_like(gates)
    gout = torch.randn_like(tokens)
    assert mo._combine_kernel_ok(xbins, gates, src, valid, tokens, K)
    assert mo._bins_bwd_kernel_ok(gbins, ggates, src, valid, tokens, K)
    assert mo._combine_bwd_kernel_ok(gout, xbins, gates, src, valid, K)

    T, B = 2 * N * K * C, 2 * E * cap * C
    calls = {
        "moe_bins": (T + B, lambda: ed.moe_bins(tokens, topi, topv, E,
                                                factor)),
        "moe_combine": (T + T // K, lambda: ed.moe_combine(
            xbins, gates, src, valid, tokens, K)),
        "moe_bins_bwd": (T + T // K, lambda: ed.moe_bins_bwd(
            gbins, ggates, src, valid, tokens, K)),
        "moe_combine_bwd": (2 * T + B, lambda: ed.moe_combine_bwd(
            gout, xbins, gates, src, valid, K)),
    }
    pool = torch.randn(max(b for b, _ in calls.values()) // 4 + 8,
                       device="cuda").to(bf)
    dst = torch.empty_like(pool)

    def copy_of(nbytes):
        n = nbytes // 4          # bf16 elements of half the bytes
        return lambda: dst[:n].copy_(pool[:n])

    cfgs = {}
    for op, (nbytes, fn) in calls.items():
        cfgs[op, "kernel"] = fn
        cfgs[op, "aten"] = aten(fn)
        cfgs[op, "copy"] = copy_of(nbytes)
    for fn in cfgs.values():
        for _ in range(args.warm_iters):
            fn()
    torch.cuda.synchronize()
    times = {c: [] for c in cfgs}
    for _ in range(args.repeats):
        for c, fn in cfgs.items():   # alternate configs inside a repeat
            times[c].append(event_us(fn, args.iters))

    summary = {"shape": name}
    for (op, cfg), xs in times.items():
        med = statistics.median(xs)
        nbytes = calls[op][0]
        print(json.dumps({
            "shape": name, "dims": {"N": N, "C": C, "E": E, "K": K,
                                    "cap": cap},
            "op": op, "config": cfg, "bytes": nbytes,
            "us": {"med": round(med, 2), "min": round(min(xs), 2),
                   "max": round(max(xs), 2)},
            "tbps": round(nbytes / med / 1e6, 4)}), flush=True)
        summary[f"{op}_{cfg}_us"] = round(med, 1)
    for op in OPS:
        summary[f"{op}_aten_over_kernel_time"] = round(
            summary[f"{op}_aten_us"] / summary[f"{op}_kernel_us"], 2)
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="",
                    help="N,C,E,K,factor; default: MIXTRAL_SMALL's shape")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warm-iters", type=int, default=20)
    args = ap.parse_args()

    assert ops.load_extension() is not None and torch.cuda.is_available(), \
        "bench_moe_routing needs the HIP extension and a GPU"
    shapes = SHAPES
    if args.shape:
        f = args.shape.split(",")
        shapes = {"custom": tuple(int(s) for s in f[:4]) + (float(f[4]),)}
    for name, shape in shapes.items():
        bench_shape(name, shape, args)


if __name__ == "__main__":
    main()
