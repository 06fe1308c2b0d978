#!/usr/bin/env python3
"""The SwiGLU kernels (csrc/swiglu_kernels.hip) against a device-to-device
copy of the same bytes and against the aten chain they replace.

Configurations, on bf16 gate, up and grad of one shape (T bytes each):

  swiglu_fwd    swiglu(gate, up): reads 2 T, writes 1 T
  swiglu_bwd    swiglu_bwd(grad, gate, up): reads 3 T, writes 2 T
  copy_fwd      a copy of 1.5 T: the same 3 T of traffic, the yardstick
  copy_bwd      a copy of 2.5 T: the same 5 T
  aten_fwd      F.silu(gate) * up: two kernels, 5 T
  aten_bwd      its autograd backward (mul, mul, silu_backward): 9 T

Shapes: the Mixtral expert activation [8, 2560, 14336] (8 experts, capacity
2560 for 8192 tokens, ffn_hidden 14336) as two separate tensors, and a dense
[64*1024, 2048] with gate and up taken as the two halves of one [.., 4096]
projection output; or one given on the command line.

One process alternates the configurations inside each of --repeats repeats,
after a warm-up of every configuration. Times are device time from the torch
profiler, summed over every kernel a configuration launches, reported as
median [min-max] over the repeats. TB/s is 3 T (forward) or 5 T (backward)
over the median time for every configuration of that direction, whatever it
really moves. One JSON line per configuration and shape, then one summary
line per shape: the kernels' rates over the copy's and the aten chain's time
over the kernels'.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F
from torch.autograd import DeviceType

import easydist_amd.ops as ops
from easydist_amd.ops import swiglu as sw

# name -> (shape, gate and up as halves of one buffer)
SHAPES = {
    "mixtral_expert": ((8, 2560, 14336), False),
    "dense_halves": ((64 * 1024, 2048), True),
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


def bench_shape(name, shape, halves, args):
    torch.manual_seed(0)
    if halves:
        h = torch.randn(shape[:-1] + (2 * shape[-1],), device="cuda") \
            .to(torch.bfloat16)
        gate, up = h.chunk(2, -1)
    else:
        gate = torch.randn(shape, device="cuda").to(torch.bfloat16)
        up = torch.randn(shape, device="cuda").to(torch.bfloat16)
    grad = torch.randn(shape, device="cuda").to(torch.bfloat16)
    assert sw._kernel_ok(grad, gate, up)
    n = grad.numel()
    T = 2 * n
    src = torch.randn(5 * n // 2, device="cuda").to(torch.bfloat16)
    dst = torch.empty_like(src)
    # the aten chain's autograd graph, built once: the backward is timed
    # alone
    ga = gate.detach().requires_grad_(True)
    ua = up.detach().requires_grad_(True)
    ya = F.silu(ga) * ua
    ed = torch.ops.easydist_amd

    cfgs = {
        "swiglu_fwd": (3, lambda: ed.swiglu(gate, up)),
        "copy_fwd": (3, lambda: dst[:3 * n // 2].copy_(src[:3 * n // 2])),
        "aten_fwd": (3, lambda: F.silu(gate) * up),
        "swiglu_bwd": (5, lambda: ed.swiglu_bwd(grad, gate, up)),
        "copy_bwd": (5, lambda: dst.copy_(src)),
        "aten_bwd": (5, lambda: torch.autograd.grad(
            ya, (ga, ua), grad, retain_graph=True)),
    }
    for _, fn in cfgs.values():
        for _ in range(args.warm_iters):
            fn()
    torch.cuda.synchronize()
    total = {c: [] for c in cfgs}
    for _ in range(args.repeats):
        for c, (_, fn) in cfgs.items():  # alternate configs inside a repeat
            total[c].append(device_us(fn, args.iters))

    res = {}
    for c, (passes, _) in cfgs.items():
        st = stats(total[c])
        res[c] = st
        print(json.dumps({
            "shape": name, "dims": list(shape), "halves": halves,
            "config": c, "device_us": st, "bytes": passes * T,
            "tbps": round(passes * T / st["med"] / 1e6, 3)}), flush=True)
    print(json.dumps({
        "shape": name,
        "swiglu_fwd_over_copy_rate": round(res["copy_fwd"]["med"]
                                           / res["swiglu_fwd"]["med"], 3),
        "swiglu_bwd_over_copy_rate": round(res["copy_bwd"]["med"]
                                           / res["swiglu_bwd"]["med"], 3),
        "aten_over_swiglu_fwd_time": round(res["aten_fwd"]["med"]
                                           / res["swiglu_fwd"]["med"], 2),
        "aten_over_swiglu_bwd_time": round(res["aten_bwd"]["med"]
                                           / res["swiglu_bwd"]["med"], 2),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="",
                    help="d0,d1,..,F as separate tensors; default: the two "
                         "named shapes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm-iters", type=int, default=10)
    args = ap.parse_args()

    assert ops.load_extension() is not None and torch.cuda.is_available(), \
        "bench_swiglu needs the HIP extension and a GPU"
    shapes = SHAPES
    if args.shape:
        shapes = {"custom": (tuple(int(s) for s in args.shape.split(",")),
                             False)}
    for name, (shape, halves) in shapes.items():
        bench_shape(name, shape, halves, args)


if __name__ == "__main__":
    main()
