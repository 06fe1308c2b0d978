#!/usr/bin/env python3
"""Flash attention kernel timing: fwd, dq and dkv, causal and not, under
both workgroup maps (EASYDIST_ATTN_MAP) and both LDS forms
(EASYDIST_ATTN_TR: 1 = one image per tile read transposed, 0 = the second
transposed copy) and both dkv workgroup geometries (EASYDIST_DKV_GEOM: 0 =
8 waves on 128 keys, 1 = 4 waves on 64 keys with the half-tile loop); the
launch code reads all three at every call, so one process can alternate
them.

Event timings give fwd and total bwd (delta + dq + dkv).  Per-kernel
figures for dq and dkv come from a kernel trace: either run this script
under `rocprofv3 --kernel-trace --stats` with one --map and one --causal
value, in a run of its own, or pass --per-kernel to collect them with the
torch profiler in-process (attributed per configuration).

Every configuration is timed --repeats times, the maps and forms
alternated inside each repeat, and min / median / max are reported so a
difference can be set against the run-to-run spread.  One JSON line per
configuration.

--ragged times a shape set of its own instead (S % 128 != 0, see
run_ragged); without it the output is what it always was.  --kv-heads N
times grouped-query attention against the expand-and-reduce a build
without the GQA kernels needs (see run_gqa).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import easydist_amd.ops as ops

SHAPES = [(64, 12, 1024, 64), (16, 16, 2048, 128),
          (64, 12, 1152, 64)]   # nblk = 9: legacy map is naturally mixed

# --ragged only (never part of "all" above): ((B, H, S, D), causal) with
# S % 128 != 0; EASYDIST_ATTN_TR does not apply to these
RAGGED_SHAPES = [((256, 16, 197, 64), False),    # ViT-Large
                 ((64, 12, 1000, 64), True)]

# report name -> substring of the kernel's name in a trace
KERNELS = {"fwd": "flash_fwd", "dq": "flash_bwd_dq", "dkv": "flash_bwd_dkv",
           "delta": "attn_delta"}


def time_ms(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def kernel_ms(fn, iters):
    """Mean device time per call of each flash kernel, via the profiler."""
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
        for tag in KERNELS.values():
            if tag in ev.key:
                us = getattr(ev, "device_time_total", None)
                if us is None:
                    us = ev.cuda_time_total
                if us:
                    out[tag] = out.get(tag, 0.0) + us / 1e3 / iters
    return out


def stats(xs):
    return {"min": min(xs), "med": statistics.median(xs), "max": max(xs),
            "all": [round(x, 4) for x in xs]}   # in measurement order


def run_ragged(args):
    """--ragged: the public op, forward + backward, at each ragged shape
    and at the next S that is a multiple of 128, alternated inside each
    repeat.  The public op, not the extension, so the same script also
    times a build whose kernels refuse these shapes (aten math path).
    peak_mib: peak allocated memory of one forward + backward above what
    the inputs hold."""
    from easydist_amd.ops.attention import scaled_dot_product_attention
    picked = RAGGED_SHAPES if args.shapes == "all" else \
        [RAGGED_SHAPES[int(i)] for i in args.shapes.split(",")]
    for (B, H, S, D), causal in picked:
        S_al = (S + 127) // 128 * 128
        cfgs = {}
        for s in (S, S_al):
            q, k, v = (torch.randn(B, H, s, D, device="cuda",
                                   dtype=torch.bfloat16, requires_grad=True)
                       for _ in range(3))
            g = torch.randn(B, H, s, D, device="cuda", dtype=torch.bfloat16)

            def step(q=q, k=k, v=v, g=g):
                scaled_dot_product_attention(q, k, v, causal=causal) \
                    .backward(g)
                q.grad = k.grad = v.grad = None
            cfgs[s] = step
        times = {s: [] for s in cfgs}
        peak = {}
        for s, step in cfgs.items():
            time_ms(step, args.warm_iters, 0)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            peak[s] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for _ in range(args.repeats):
            for s, step in cfgs.items():    # alternate inside a repeat
                times[s].append(time_ms(step, args.iters))
        for s in cfgs:
            r = {"shape": f"B{B} H{H} S{s} D{D}", "causal": int(causal),
                 "ragged": int(s % 128 != 0), "op": "public fwd+bwd",
                 "fwd_bwd_ms": stats(times[s]),
                 "peak_mib": round(peak[s], 1)}
            if s != S_al:
                r["vs_next_aligned"] = (statistics.median(times[s])
                                        / statistics.median(times[S_al]))
            print(json.dumps(r), flush=True)


def run_gqa(args, ext):
    """--kv-heads: grouped-query attention, forward + backward through the
    extension, with K/V of --kv-heads heads.  Two steps alternated inside
    each repeat: "gqa", the kernels on [B, Hkv, S, D] K/V, and "expand",
    what a build without them has to do: repeat_interleave K/V to H heads,
    the MHA kernels, and a sum of dk/dv over each group.  --per-kernel adds
    the device time of each flash kernel of the gqa step (the dkv grid is
    ceil(S/128) * B * Hkv workgroups: an under-filled chip shows there)."""
    shapes = [tuple(int(x) for x in s.split(","))
              for s in args.gqa_shapes.split(";")]
    causals = {"0": [False], "1": [True], "both": [True, False]}[args.causal]
    Hkv = args.kv_heads
    for (B, H, S, D) in shapes:
        assert H % Hkv == 0, (H, Hkv)
        G = H // Hkv
        bf = torch.bfloat16
        q = torch.randn(B, H, S, D, device="cuda", dtype=bf)
        g = torch.randn_like(q)
        k = torch.randn(B, Hkv, S, D, device="cuda", dtype=bf)
        v = torch.randn_like(k)
        for causal in causals:
            def gqa():
                o, lse = ext.flash_attn_fwd(q, k, v, causal)
                return ext.flash_attn_bwd(g, q, k, v, o, lse, causal)

            def expand():
                ke = k.repeat_interleave(G, dim=1)
                ve = v.repeat_interleave(G, dim=1)
                o, lse = ext.flash_attn_fwd(q, ke, ve, causal)
                dq, dk, dv = ext.flash_attn_bwd(g, q, ke, ve, o, lse, causal)
                return (dq, dk.view(B, Hkv, G, S, D).sum(2),
                        dv.view(B, Hkv, G, S, D).sum(2))

            steps = {"gqa": gqa, "expand": expand}
            times = {n: [] for n in steps}
            for fn in steps.values():
                time_ms(fn, args.warm_iters, 0)
            for _ in range(args.repeats):
                for n, fn in steps.items():   # alternate inside a repeat
                    times[n].append(time_ms(fn, args.iters))
            r = {"shape": f"B{B} H{H} Hkv{Hkv} S{S} D{D}",
                 "causal": int(causal),
                 "dkv_workgroups": (S + 127) // 128 * B * Hkv,
                 "fwd_bwd_ms": {n: stats(xs) for n, xs in times.items()}}
            r["gqa_vs_expand"] = (statistics.median(times["gqa"])
                                  / statistics.median(times["expand"]))
            if args.per_kernel:
                km = kernel_ms(gqa, args.iters)
                r["kernel_ms"] = {n: round(km[tag], 4)
                                  for n, tag in KERNELS.items() if tag in km}
            print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-heads", type=int, default=0,
                    help="time grouped-query attention with this many K/V "
                         "heads against repeat_interleave + the MHA kernels "
                         "(see run_gqa); shapes from --gqa-shapes")
    ap.add_argument("--gqa-shapes", default="4,32,2048,128;4,32,2048,64",
                    help="--kv-heads only: B,H,S,D;B,H,S,D;...")
    ap.add_argument("--ragged", action="store_true",
                    help="time the public op fwd+bwd at the ragged shapes "
                         "(ViT-L S = 197 full, S = 1000 causal) and at the "
                         "next aligned S; --shapes then indexes that list")
    ap.add_argument("--causal", choices=["0", "1", "both"], default="1")
    ap.add_argument("--map", choices=["0", "1", "both", "env"], default="env",
                    help="workgroup map: 0 legacy, 1 balanced, both = "
                         "alternate them, env = leave EASYDIST_ATTN_MAP alone")
    ap.add_argument("--tr", choices=["0", "1", "both", "env"], default="env",
                    help="LDS form: 0 transposed copy, 1 transposed reads, "
                         "both = alternate them, env = leave EASYDIST_ATTN_TR "
                         "alone (unset: each kernel's shipped default)")
    ap.add_argument("--dkv-geom", choices=["0", "1", "both", "env"],
                    default="env",
                    help="dkv geometry: 0 = 8 waves per 128-key block, 1 = 4 "
                         "waves per 64-key block, both = alternate them, env "
                         "= leave EASYDIST_DKV_GEOM alone (unset: the shipped "
                         "default per head size)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm-iters", type=int, default=50)
    ap.add_argument("--shapes", default="all",
                    help="comma-separated indices into the shape list")
    ap.add_argument("--bhsd", default=None,
                    help="B,H,S,D[,Hkv];... : time these shapes through the "
                         "extension instead of the --shapes list; any S, and "
                         "K/V of Hkv heads when given (EASYDIST_ATTN_TR does "
                         "not apply to ragged S or Hkv != H)")
    ap.add_argument("--per-kernel", action="store_true",
                    help="also report per-kernel device time (torch profiler)")
    args = ap.parse_args()

    ext = ops.load_extension()
    assert ext is not None
    if args.ragged:
        return run_ragged(args)
    if args.kv_heads:
        return run_gqa(args, ext)
    causals = {"0": [False], "1": [True], "both": [True, False]}[args.causal]
    pick = {"0": ["0"], "1": ["1"], "both": ["0", "1"], "env": [None]}
    # a configuration is a (map, tr, dkv geometry) triple
    maps = [(m, t, g) for m in pick[args.map] for t in pick[args.tr]
            for g in pick[args.dkv_geom]]
    shapes = SHAPES if args.shapes == "all" else \
        [SHAPES[int(i)] for i in args.shapes.split(",")]
    if args.bhsd:
        shapes = [tuple(int(x) for x in s.split(","))
                  for s in args.bhsd.split(";")]

    def set_map(cfg):
        m, t, g = cfg
        if m is not None:
            os.environ["EASYDIST_ATTN_MAP"] = m
        if t is not None:
            os.environ["EASYDIST_ATTN_TR"] = t
        if g is not None:
            os.environ["EASYDIST_DKV_GEOM"] = g

    for (B, H, S, D, *kvh) in shapes:
        Hkv = kvh[0] if kvh else H
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
        g = torch.randn_like(q)
        for causal in causals:
            o, lse = ext.flash_attn_fwd(q, k, v, causal)
            fwd = lambda: ext.flash_attn_fwd(q, k, v, causal)
            bwd = lambda: ext.flash_attn_bwd(g, q, k, v, o, lse, causal)
            t_fwd = {m: [] for m in maps}
            t_bwd = {m: [] for m in maps}
            t_k = {m: {n: [] for n in KERNELS} for m in maps}
            # bring clocks and caches to steady state before the first
            # repeat: without this the first repeat of a configuration
            # reads ~10% high and sets the whole min-max spread
            for m in maps:
                set_map(m)
                time_ms(fwd, args.warm_iters, 0)
                time_ms(bwd, args.warm_iters, 0)
            for _ in range(args.repeats):
                for m in maps:          # alternate configs inside a repeat
                    set_map(m)
                    t_fwd[m].append(time_ms(fwd, args.iters))
                    t_bwd[m].append(time_ms(bwd, args.iters))
                    if args.per_kernel:
                        km = kernel_ms(fwd, args.iters)
                        km.update(kernel_ms(bwd, args.iters))
                        for n, tag in KERNELS.items():
                            if tag in km:
                                t_k[m][n].append(km[tag])
            # matmul flops the fwd does: QK^T + PV, halved under the mask
            fl_fwd = 2.0 * B * H * S * S * D * 2 * (0.5 if causal else 1.0)
            fl_bwd = fl_fwd * 2.5       # model flops of the backward
            for m in maps:
                r = {"shape": f"B{B} H{H} S{S} D{D}"
                     + (f" Hkv{Hkv}" if Hkv != H else ""),
                     "causal": int(causal),
                     "map": m[0] if m[0] is not None
                     else os.environ.get("EASYDIST_ATTN_MAP", "1"),
                     "tr": m[1] if m[1] is not None
                     else os.environ.get("EASYDIST_ATTN_TR", "default"),
                     "dkv_geom": m[2] if m[2] is not None
                     else os.environ.get("EASYDIST_DKV_GEOM", "default"),
                     "fwd_ms": stats(t_fwd[m]), "bwd_ms": stats(t_bwd[m])}
                r["fwd_tf"] = fl_fwd / r["fwd_ms"]["med"] / 1e9
                r["bwd_tf"] = fl_bwd / r["bwd_ms"]["med"] / 1e9
                if args.per_kernel:
                    r["kernel_ms"] = {n: stats(xs)
                                      for n, xs in t_k[m].items() if xs}
                    # executed matmuls: fwd 2, dq 3 (S, dP, dQ), dkv 4
                    # (S^T, dV, dP^T, dK) -> 1.5x and 2x the fwd flops
                    r["kernel_tf"] = {
                        n: fl_fwd * f / r["kernel_ms"][n]["med"] / 1e9
                        for n, f in (("fwd", 1.0), ("dq", 1.5), ("dkv", 2.0))
                        if n in r["kernel_ms"]}
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
