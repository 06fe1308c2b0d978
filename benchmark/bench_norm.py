#!/usr/bin/env python3
"""LayerNorm kernels around the residual stream: the unfused kernel groups
against the residual-fused kernels (csrc/norm_kernels.hip).

Configurations (all on [rows, dim] bf16, one pass over a tensor = "1 T"):

  fwd_unfused    aten add (3 T) + norm_fwd (2 T)
  fwd_fused      add_norm_fwd: read a, b; write sum, out (4 T)
  bwd_unfused    norm_bwd (3 T) + norm_param_grads (2 T) + aten add (3 T),
                 plus the two at::zeros fills      (EASYDIST_NORM_FUSE=0)
  bwd_fused_res  norm_bwd_fused with a residual (4 T) + partials sum
  bwd_fused      norm_bwd_fused without one (3 T) + partials sum
  bwd_fused_res@G  the same at G blocks (--blocks, EASYDIST_NORM_BWD_BLOCKS)

The launch code reads both knobs at every call, so one process alternates
the configurations inside each of --repeats repeats, after a warm-up of
every configuration. Times are device time from the torch profiler, summed
over every kernel a configuration launches and listed per kernel, reported
as median [min-max] over the repeats. TB/s is the configuration's bytes (as
counted above, plus the fp32 partials) over its median time. One JSON line
per configuration, then one line that sets each fused configuration against
the group it replaces: the gain counts when it exceeds 3x the unfused
group's max-min spread.
"""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
from torch.autograd import DeviceType

import easydist_amd.ops as ops

EPS = 1e-5


def default_blocks(dim):
    """norm_bwd_blocks() in csrc/norm_kernels.hip."""
    return 1024 if dim <= 512 else 768 if dim <= 1024 else 256


def kernel_us(fn, iters):
    """Device us per call of every kernel fn launches: {name: us}."""
    acts = [torch.profiler.ProfilerActivity.CPU,
            torch.profiler.ProfilerActivity.CUDA]
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=acts) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        if ev.device_type != DeviceType.CUDA:
            continue
        us = getattr(ev, "self_device_time_total", None)
        if us is None:
            us = ev.self_cuda_time_total
        if us:
            # aten elementwise kernels differ only in their functor
            m = re.search(r"\w*Functor\w*", ev.key)
            name = m.group(0) if m else \
                ev.key.split("(")[0].split("<")[0].split(" ")[-1]
            out[name] = out.get(name, 0.0) + us / iters
    return out


def stats(xs):
    return {"med": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--blocks", default="",
                    help="comma-separated grid sizes of the fused backward "
                         "to sweep, e.g. 256,512,768,1024,2048")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm-iters", type=int, default=50)
    args = ap.parse_args()

    ext = ops.load_extension()
    assert ext is not None and torch.cuda.is_available(), \
        "bench_norm needs the HIP extension and a GPU"
    R, D = args.rows, args.dim
    rnd = lambda *s: torch.randn(*s, device="cuda").bfloat16()
    a, b, grad, res, w, bias = (rnd(R, D), rnd(R, D), rnd(R, D), rnd(R, D),
                                rnd(D), rnd(D))
    x = a + b
    _, mean, rstd = ext.layer_norm_fwd(x, w, bias, EPS)
    mask = [True, True, True]
    T = R * D * 2

    def bwd_unfused():
        dx, dw, db = ext.layer_norm_bwd(grad, x, mean, rstd, w, mask)
        return torch.add(res, dx), dw, db

    def partials(G):
        g = min(G, (R + 3) // 4)
        return g * 2 * D * 4 * 2      # written, then read by the sum kernel

    # name -> (env, fn, bytes)
    cfgs = {
        "fwd_unfused": ({}, lambda: ext.layer_norm_fwd(a + b, w, bias, EPS),
                        5 * T),
        "fwd_fused": ({}, lambda: ext.add_layer_norm_fwd(a, b, w, bias, EPS),
                      4 * T),
        "bwd_unfused": ({"EASYDIST_NORM_FUSE": "0"}, bwd_unfused, 8 * T),
        "bwd_fused_res": ({}, lambda: ext.layer_norm_bwd_res(
            grad, x, mean, rstd, w, res, mask),
            4 * T + partials(default_blocks(D))),
        "bwd_fused": ({}, lambda: ext.layer_norm_bwd(
            grad, x, mean, rstd, w, mask), 3 * T + partials(default_blocks(D))),
    }
    for G in [int(s) for s in args.blocks.split(",") if s]:
        cfgs[f"bwd_fused_res@{G}"] = (
            {"EASYDIST_NORM_BWD_BLOCKS": str(G)}, cfgs["bwd_fused_res"][1],
            4 * T + partials(G))

    def run(name, iters, profile):
        env, fn, _ = cfgs[name]
        for k in ("EASYDIST_NORM_FUSE", "EASYDIST_NORM_BWD_BLOCKS"):
            os.environ.pop(k, None)
        os.environ.update(env)
        if profile:
            return kernel_us(fn, iters)
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()

    for name in cfgs:
        run(name, args.warm_iters, False)
    total = {n: [] for n in cfgs}
    per_k = {n: {} for n in cfgs}
    for _ in range(args.repeats):
        for name in cfgs:               # alternate configs inside a repeat
            ks = run(name, args.iters, True)
            total[name].append(sum(ks.values()))
            for k, us in ks.items():
                per_k[name].setdefault(k, []).append(us)

    res_json = {}
    for name, (_, _, nbytes) in cfgs.items():
        st = stats(total[name])
        res_json[name] = st
        print(json.dumps({
            "config": name, "rows": R, "dim": D, "device_us": st,
            "bytes": nbytes, "tbps": round(nbytes / st["med"] / 1e6, 2),
            "kernels_us": {k: stats(v) for k, v in per_k[name].items()}}),
            flush=True)
    verdict = {}
    for fused, base in (("fwd_fused", "fwd_unfused"),
                        ("bwd_fused_res", "bwd_unfused")):
        gain = res_json[base]["med"] - res_json[fused]["med"]
        spread = res_json[base]["max"] - res_json[base]["min"]
        verdict[fused] = {"gain_us": round(gain, 2),
                          "unfused_spread_us": round(spread, 2),
                          "established": gain > 3 * spread}
    print(json.dumps({"verdict": verdict}), flush=True)


if __name__ == "__main__":
    main()
