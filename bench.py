#!/usr/bin/env python3
"""Flagship training benchmark: GPT-2 train-step throughput (samples/sec).

Driver contract:
  python bench.py --gpus N --steps K --warmup W
N>1 is launched via torch.distributed.run with one rank per GPU over RCCL.
Measures the BASELINE.json headline: train-step throughput (samples/sec,
whole node) for GPT-2 under easydist_amd auto-SPMD, bf16 autocast,
synthetic data, random-init weights; also reports the strategy-search
wallclock. Weak scaling: per-GPU batch fixed, global batch = B * N.

A plain run sets up, warms up, times --steps train steps and prints one
JSON result line; that is everything the headline figure needs.
  --dump-outputs DIR  after the timed steps, write what the last timed
                      step computed as DIR/<name>.npy (float32): the loss
                      the caller receives and a fixed, seeded sample of the
                      parameters the step updated. Inputs and
                      initial weights are seeded, so two builds run with the
                      same arguments can be compared output for output.
  --full              also run the secondary measurements and checks. The
                      benchmark has none of its own today (the comparison
                      harnesses live in benchmark/), so the flag changes
                      nothing yet; anything added later that the headline
                      figure does not need goes behind it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


def _comm_summary(compiled):
    """Count the collectives the solver's strategy put in ONE step —
    the honest description of what 'auto' chose at this world size."""
    try:
        rts = list(getattr(compiled, "compiled", {}).values())
        if not rts or not hasattr(rts[0], "gm"):
            return None
        from collections import Counter
        cnt = Counter()
        for n in rts[0].gm.graph.nodes:
            t = getattr(n.target, "__name__", "")
            if t.startswith("rt_") and t.endswith("_start"):
                cnt[t[3:-6]] += 1
        return dict(cnt) or None
    except Exception:
        return None


# --dump-outputs: elements sampled per parameter tensor (GPT-2 small has
# 149 of them -> ~2.4 MB of float32); the whole sample stays under 64 MB
_DUMP_PER_PARAM = 4096
_DUMP_MAX_ELEMS = 15 * 1024 * 1024
_DUMP_SEED = 20240


def _dump_outputs(out_dir, loss, compiled, rank):
    """Write the last timed step's results as float32 .npy files."""
    import numpy as np
    # the compiled step keeps the trained parameters in its own state;
    # compiled.named_parameters() is how a caller reads them back (it
    # gathers shards, so every rank takes part and rank 0 writes)
    named = compiled.named_parameters()
    if rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().to(torch.float32).cpu().numpy())
    # the same seeded positions are sampled in every run
    g = torch.Generator(device="cpu").manual_seed(_DUMP_SEED)
    per_param = max(1, min(_DUMP_PER_PARAM,
                           _DUMP_MAX_ELEMS // max(len(named), 1)))
    parts = []
    for prm in named.values():
        flat = prm.detach().reshape(-1)
        if flat.numel() > per_param:
            pos = torch.randint(0, flat.numel(), (per_param,), generator=g)
            flat = flat[pos.to(flat.device)]
        parts.append(flat.to(torch.float32).cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"),
            torch.cat(parts).numpy())


def _parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="gpt2-small",
                   choices=["gpt2-small", "gpt2-medium", "gpt2-1.3b",
                            "gpt-1l-12288", "vit-large", "mixtral-4l",
                            "mixtral-small"])
    p.add_argument("--per-gpu-batch", type=int, default=64)   # fills 256 CUs (sweep: 8->314, 32->394, 64->415 samples/s)
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--parallel", default="auto")
    # eager is currently faster than hipGraph capture+replay: the fused
    # multi-tensor Adam kernel is capture-unsafe (chunk-table upload) and
    # capture falls back to the decomposed per-param math
    p.add_argument("--hipgraph", action="store_true")
    p.add_argument("--no-hipgraph", action="store_true")   # back-compat
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs as DIR/*.npy")
    p.add_argument("--full", action="store_true",
                   help="also run secondary measurements (none today)")
    args = p.parse_args(argv)
    if args.steps < 1:
        p.error("--steps must be at least 1")
    return args


def main():
    args = _parse_args()

    import torch.distributed as dist

    from easydist_amd import easydist_compile, easydist_setup, set_device_mesh
    from easydist_amd.models import gpt as gptm

    world_size = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    n_gpus = max(world_size, 1)
    use_cuda = torch.cuda.is_available()
    device = f"cuda:{local_rank}" if use_cuda else "cpu"
    # the pluggable allocator (EASYDIST_MEM_OPT) must be swapped in
    # BEFORE anything initializes the CUDA context
    easydist_setup(backend="torch", device="cuda" if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(local_rank)

    backend = "nccl" if use_cuda else "gloo"
    if world_size > 1:
        dist.init_process_group(backend=backend)
    else:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        dist.init_process_group(backend=backend, rank=0, world_size=1)
    set_device_mesh(list(range(world_size)), ["spmd0"])

    global_batch = args.per_gpu_batch * n_gpus
    torch.manual_seed(1234 + 0)   # same weights everywhere
    g = torch.Generator(device="cpu").manual_seed(7)     # same on all ranks

    if args.model == "vit-large":
        # BASELINE config #4: ViT-Large, mixed DP+TP reshard
        from easydist_amd.models import vit as vitm
        model = vitm.ViT(vitm.VIT_LARGE).to(device)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=use_cuda)

        def train_step(model, opt, x, y):
            return vitm.vit_train_step(model, opt, x, y)
        idx = torch.randn(global_batch, 3, 224, 224, generator=g).to(device)
        tg = torch.randint(0, 1000, (global_batch,), generator=g).to(device)
        tokens_per_sample = (224 // 16) ** 2 + 1
    elif args.model.startswith("mixtral"):
        # BASELINE config #5: Mixtral-shape MoE, expert all-to-all; module
        # EP over the world group when world>1
        from easydist_amd.models import moe as moem
        cfg = (moem.MIXTRAL_BENCH_4L if args.model == "mixtral-4l"
               else moem.MIXTRAL_SMALL)
        if args.seq != cfg.block_size:
            from dataclasses import replace
            cfg = replace(cfg, block_size=args.seq)
        # EP is chosen by the auto-SPMD solver (ops/moe_ops.py); the
        # module-level ep_group path stays available for eager reference
        model = moem.MoEGPT(cfg, ep_group=None).to(device)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=use_cuda)

        def train_step(model, opt, idx, targets):
            return moem.moe_train_step(model, opt, idx, targets)
        seq = cfg.block_size
        idx = torch.randint(0, cfg.vocab_size, (global_batch, seq),
                            generator=g).to(device)
        tg = torch.randint(0, cfg.vocab_size, (global_batch, seq),
                           generator=g).to(device)
        tokens_per_sample = seq
    else:
        cfg = {
            "gpt2-small": gptm.GPT2_SMALL,
            "gpt2-medium": gptm.GPT2_MEDIUM,
            "gpt2-1.3b": gptm.GPT2_1_3B,
            "gpt-1l-12288": gptm.GPT_BENCH_1L,
        }[args.model]
        if args.seq != cfg.block_size:
            from dataclasses import replace
            cfg = replace(cfg, block_size=args.seq)
        model = gptm.GPT(cfg).to(device)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=use_cuda)

        def train_step(model, opt, idx, targets):
            return gptm.gpt_train_step(model, opt, idx, targets)
        idx = torch.randint(0, cfg.vocab_size, (global_batch, args.seq),
                            generator=g).to(device)
        tg = torch.randint(0, cfg.vocab_size, (global_batch, args.seq),
                           generator=g).to(device)
        tokens_per_sample = args.seq

    compiled = easydist_compile(train_step, parallel_mode=args.parallel,
                                cuda_graph=args.hipgraph)

    t_compile = time.time()
    for _ in range(max(args.warmup, 1)):
        loss = compiled(model, opt, idx, tg)
    if use_cuda:
        torch.cuda.synchronize()
    compile_and_warmup_s = time.time() - t_compile

    search_s = None
    for rt in compiled.compiled.values():
        if hasattr(rt, "meta"):
            search_s = rt.meta.get("search_time", 0) + rt.meta.get(
                "solve_time", 0)

    dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        loss = compiled(model, opt, idx, tg)
    if use_cuda:
        torch.cuda.synchronize()
    dist.barrier()
    elapsed = time.time() - t0
    # max over ranks
    e = torch.tensor([elapsed], device=device if use_cuda else "cpu")
    dist.all_reduce(e, op=dist.ReduceOp.MAX)
    elapsed = float(e)

    ms_per_step = elapsed / args.steps * 1000.0
    samples_per_sec = global_batch * args.steps / elapsed

    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, loss, compiled, rank)

    if rank == 0:
        family = ("vit" if args.model.startswith("vit")
                  else "mixtral_moe" if args.model.startswith("mixtral")
                  else "gpt2")
        out = {
            "metric": f"{family}_train_samples_per_sec",
            "value": samples_per_sec,
            "unit": "samples/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": global_batch,
                "seq_len": args.seq,
                "parallelism": f"{args.parallel}(dp{n_gpus})",
                "comm_per_step": _comm_summary(compiled),
                "strategy_search_s": search_s,
                "compile_warmup_s": round(compile_and_warmup_s, 2),
                "loss": float(loss) if loss is not None else None,
            },
        }
        print(json.dumps(out))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
