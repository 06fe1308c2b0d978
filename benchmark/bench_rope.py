#!/usr/bin/env python3
"""The RoPE kernel (csrc/rope_kernels.hip) against a device-to-device copy of
the same bytes and against the aten formula.

Configurations, on bf16 qkv [B, S, W], W = (H + 2*Hkv)*D:

  rope_fwd      rope_qkv, inverse=False
  rope_inv      rope_qkv, inverse=True (the backward)
  copy          out.copy_(qkv): reads and writes the same 2*B*S*W*2 bytes, the
                yardstick: the kernel moves a copy's traffic plus table reads
                that should stay in cache
  aten          the same formula as slice/mul/sub/cat chains (ops/rope._math)

Shapes: GPT-2 small (B=64, S=1024, H=Hkv=12, D=64) and the Mixtral GQA shape
(B=4, S=2048, H=32, Hkv=8, D=128), or one given on the command line.

One process alternates the configurations inside each of --repeats repeats,
after a warm-up of every configuration. Times are device time from the torch
profiler, summed over every kernel a configuration launches, reported as
median [min-max] over the repeats. GB/s is 2*B*S*W*2 bytes over the median
time for every configuration, whatever it really moves. One JSON line per
configuration and shape, then one summary line per shape: the kernel's rate
over the copy's, and what the v columns cost: they are Hkv/(H + 2*Hkv) of
the bytes (a third for MHA), copied through so that the packed layout
survives.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
from torch.autograd import DeviceType

import easydist_amd.ops as ops
from easydist_amd.ops import rope

SHAPES = {
    "gpt2_small": (64, 1024, 12, 12, 64),
    "mixtral_gqa": (4, 2048, 32, 8, 128),
}


def device_us(fn, iters):
    """Device us per call, summed over every kernel fn launches."""
    acts = [torch.profiler.ProfilerActivity.CPU,
            torch.profiler.ProfilerActivity.CUDA]
    with torch.profiler.profile(activities=acts) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    total = 0.0
    for ev in prof.key_averages():
        if ev.device_type != DeviceType.CUDA:
            continue
        us = getattr(ev, "self_device_time_total", None)
        if us is None:
            us = ev.self_cuda_time_total
        total += us / iters
    return total


def stats(xs):
    return {"med": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2)}


def bench_shape(name, shape, args):
    B, S, H, Hkv, D = shape
    W = (H + 2 * Hkv) * D
    torch.manual_seed(0)
    qkv = torch.randn(B, S, W, device="cuda").to(torch.bfloat16)
    out = torch.empty_like(qkv)
    cos, sin = rope.rope_tables(S, D, device="cuda")
    op = torch.ops.easydist_amd.rope_qkv
    assert rope._kernel_ok(qkv, cos, sin)
    nbytes = 2 * B * S * W * 2

    cfgs = {
        "rope_fwd": lambda: op(qkv, cos, sin, H, Hkv, False),
        "rope_inv": lambda: op(qkv, cos, sin, H, Hkv, True),
        "copy": lambda: out.copy_(qkv),
        "aten": lambda: rope._math(qkv, cos, sin, H, Hkv, False),
    }
    for fn in cfgs.values():
        for _ in range(args.warm_iters):
            fn()
    torch.cuda.synchronize()
    total = {n: [] for n in cfgs}
    for _ in range(args.repeats):
        for n, fn in cfgs.items():      # alternate configs inside a repeat
            total[n].append(device_us(fn, args.iters))

    res = {}
    for n in cfgs:
        st = stats(total[n])
        res[n] = st
        print(json.dumps({
            "shape": name, "B": B, "S": S, "H": H, "Hkv": Hkv, "D": D,
            "config": n, "device_us": st, "bytes": nbytes,
            "gbps": round(nbytes / st["med"] / 1e3, 1)}), flush=True)
    v_frac = Hkv / (H + 2 * Hkv)
    print(json.dumps({
        "shape": name,
        "rope_fwd_over_copy_rate": round(res["copy"]["med"]
                                         / res["rope_fwd"]["med"], 3),
        "rope_inv_over_copy_rate": round(res["copy"]["med"]
                                         / res["rope_inv"]["med"], 3),
        "aten_over_rope_fwd_time": round(res["aten"]["med"]
                                         / res["rope_fwd"]["med"], 2),
        "v_column_byte_fraction": round(v_frac, 4),
        "v_column_us_at_rope_fwd_rate": round(v_frac
                                              * res["rope_fwd"]["med"], 2),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="",
                    help="B,S,H,Hkv,D; default: the two named shapes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm-iters", type=int, default=20)
    args = ap.parse_args()

    assert ops.load_extension() is not None and torch.cuda.is_available(), \
        "bench_rope needs the HIP extension and a GPU"
    shapes = SHAPES
    if args.shape:
        shapes = {"custom": tuple(int(s) for s in args.shape.split(","))}
    for name, shape in shapes.items():
        bench_shape(name, shape, args)


if __name__ == "__main__":
    main()
