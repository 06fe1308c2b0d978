"""lower_norm_residual_fuse: residual adds folded into the LayerNorm ops.

CPU-executable: the fused ops' CPU impls compose the same aten calls as
the unfused graph, so losses must match exactly (the GPU kernels are
covered by tests/test_gpu_norm_fuse.py).
"""
import operator

import torch
import torch.fx as fx

N_LAYER = 2


def _compile_tiny_gpt():
    from easydist_amd import easydist_compile, easydist_setup, \
        set_device_mesh
    from easydist_amd.models import gpt as gptm
    from easydist_amd.utils.testing import init_single_process

    init_single_process()
    easydist_setup(backend="torch", device="cpu")
    set_device_mesh([0], ["spmd0"])
    torch.manual_seed(0)
    cfg = gptm.GPTConfig(vocab_size=128, n_layer=N_LAYER, n_head=2,
                         n_embd=32, block_size=16)
    model = gptm.GPT(cfg)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    compiled = easydist_compile(gptm.gpt_train_step, cuda_graph=False)
    idx = torch.randint(0, 128, (4, 16))
    tg = torch.randint(0, 128, (4, 16))
    losses = [float(compiled(model, opt, idx, tg)) for _ in range(4)]
    gm = list(compiled.compiled.values())[0].gm
    return losses, gm


def _calls(gm, name):
    return [n for n in gm.graph.nodes if n.op == "call_function"
            and getattr(n.target, "__name__", "") == name]


def test_gpt_residual_adds_fused(monkeypatch):
    monkeypatch.delenv("EASYDIST_NORM_FUSE", raising=False)
    losses, gm = _compile_tiny_gpt()

    fwd = _calls(gm, "add_layer_norm_fwd.default")
    bwd = _calls(gm, "layer_norm_bwd_res.default")
    assert len(fwd) == 2 * N_LAYER, [n.name for n in fwd]
    assert len([n for n in bwd if n.args[5] is not None]) == 2 * N_LAYER, \
        [(n.name, n.args[5]) for n in bwd]

    # no add left that feeds a lowered LayerNorm forward, or that consumes
    # a LayerNorm dx nobody else reads
    ln_fwd_names = ("layer_norm_fwd.default", "add_layer_norm_fwd.default")
    ln_bwd_names = ("layer_norm_bwd.default", "layer_norm_bwd_res.default")
    for n in _calls(gm, "add.Tensor"):
        for u in n.users:
            assert not (getattr(u.target, "__name__", "") in ln_fwd_names
                        and u.args[0] is n), (n.name, u.name)
        for a in n.args:
            if isinstance(a, fx.Node) and a.target is operator.getitem \
                    and a.args[1] == 0 and len(a.users) == 1:
                src = getattr(a.args[0].target, "__name__", "")
                assert src not in ln_bwd_names, (n.name, a.name)

    monkeypatch.setenv("EASYDIST_NORM_FUSE", "0")
    losses_off, gm_off = _compile_tiny_gpt()
    assert not _calls(gm_off, "add_layer_norm_fwd.default")
    assert not _calls(gm_off, "layer_norm_bwd_res.default")
    assert losses == losses_off, (losses, losses_off)


def _hand_graph(alpha=None, b_shape=(4, 32)):
    """a + b -> layer_norm_fwd, and g + dx(layer_norm_bwd), by hand."""
    ops = torch.ops.easydist_amd
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16)
    kw = {} if alpha is None else {"alpha": alpha}
    g = fx.Graph()

    def ph(name, val):
        n = g.placeholder(name)
        n.meta["val"] = val
        return n

    a, b = ph("a", bf(4, 32)), ph("b", bf(*b_shape))
    grad, res = ph("grad", bf(4, 32)), ph("res", bf(*b_shape))
    w, bias = ph("w", bf(32)), ph("bias", bf(32))
    s = g.call_function(torch.ops.aten.add.Tensor, (a, b), kw)
    s.meta["val"] = bf(4, 32)
    ln = g.call_function(ops.layer_norm_fwd.default, (s, w, bias, 1e-5))
    out, mean, rstd = (g.call_function(operator.getitem, (ln, k))
                       for k in range(3))
    bwd = g.call_function(ops.layer_norm_bwd.default,
                          (grad, s, mean, rstd, w, [True, True, True]))
    dx = g.call_function(operator.getitem, (bwd, 0))
    d = g.call_function(torch.ops.aten.add.Tensor, (res, dx), kw)
    d.meta["val"] = bf(4, 32)
    g.output((out, d))
    return fx.GraphModule(torch.nn.Module(), g)


def _targets(gm):
    return [getattr(n.target, "__name__", str(n.target))
            for n in gm.graph.nodes if n.op == "call_function"]


def test_hand_graph_guards():
    from easydist_amd.compiler.passes.lower_hip import \
        lower_norm_residual_fuse

    # positive control: the plain form is rewritten, and still computes
    # what the unfused graph computes
    ref = _hand_graph()
    gm = _hand_graph()
    assert lower_norm_residual_fuse(gm) == 2
    names = _targets(gm)
    assert "add.Tensor" not in names, names
    assert "add_layer_norm_fwd.default" in names, names
    assert "layer_norm_bwd_res.default" in names, names
    torch.manual_seed(1)
    ins = [torch.randn(4, 32).bfloat16() for _ in range(4)] \
        + [torch.randn(32).bfloat16() for _ in range(2)]
    for got, want in zip(gm(*ins), ref(*ins)):
        assert torch.equal(got, want)

    # alpha on the add, or a broadcast operand: left alone
    for kwargs in ({"alpha": 2}, {"b_shape": (32,)}):
        gm = _hand_graph(**kwargs)
        before = _targets(gm)
        assert lower_norm_residual_fuse(gm) == 0, kwargs
        assert _targets(gm) == before, kwargs
