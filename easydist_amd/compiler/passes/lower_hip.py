"""Lower hot aten ops in the sharded graph to the gfx950 HIP kernels.

The autocast'd trace runs LayerNorm in fp32: every norm is wrapped in
bf16->fp32->bf16 casts (rocprof: ~290 cast kernels + aten layer_norm +
layer_norm_grad_input per GPT-2 step). This pass rewrites
``aten.native_layer_norm(_backward)`` to ``easydist_amd::layer_norm_fwd/
bwd`` (one-pass Welford / two-pass bwd HIP kernels that take bf16
directly with fp32 statistics inside), FOLDING the surrounding casts:

* an input that is ``_to_copy(x_bf16, fp32)`` feeds the kernel as x_bf16;
* a user that is ``_to_copy(out, bf16)`` reads the kernel's bf16 output
  directly;
* any remaining consumer dtype mismatch gets an explicit cast so graph
  semantics never change.
"""
from __future__ import annotations

import logging
import operator
from typing import Optional

import torch
import torch.fx as fx

from ...ops import norms as _norms  # noqa: F401  (registers the ops)
from ...ops import gemm as _gemm    # noqa: F401
from ...ops import swiglu as _swiglu  # noqa: F401

logger = logging.getLogger(__name__)

aten = torch.ops.aten
CAST_OPS = (aten._to_copy.default, aten.to.dtype)


def _val(n):
    return n.meta.get("val") if hasattr(n, "meta") else None


def _uncast(n: fx.Node, want: torch.dtype) -> Optional[fx.Node]:
    """If n is a cast of a `want`-dtype value, return the source."""
    if isinstance(n, fx.Node) and n.op == "call_function" \
            and n.target in CAST_OPS:
        src = n.args[0]
        v = _val(src)
        if isinstance(v, torch.Tensor) and v.dtype == want:
            return src
    return None


def _dtype_of(n) -> Optional[torch.dtype]:
    v = _val(n)
    return v.dtype if isinstance(v, torch.Tensor) else None


def lower_layer_norm(gm: fx.GraphModule) -> int:
    graph = gm.graph
    n_lowered = 0
    for n in list(graph.nodes):
        if n.op != "call_function":
            continue
        if n.target is aten.native_layer_norm.default:
            x, shape, w, b, eps = n.args
            if not isinstance(shape, (list, tuple)) or len(shape) != 1 \
                    or shape[0] % 8 != 0:
                continue
            x_bf = _uncast(x, torch.bfloat16)
            src = x_bf if x_bf is not None else x
            with graph.inserting_before(n):
                new = graph.call_function(
                    torch.ops.easydist_amd.layer_norm_fwd.default,
                    (src, w, b, float(eps)))
            _rewire_tuple(graph, n, new,
                          kernel_dtypes=[_dtype_of(src), torch.float32,
                                         torch.float32])
            n_lowered += 1
        elif n.target is aten.native_layer_norm_backward.default:
            grad, x, shape, mean, rstd, w, b, mask = n.args
            if not isinstance(shape, (list, tuple)) or len(shape) != 1 \
                    or shape[0] % 8 != 0:
                continue
            g_bf = _uncast(grad, torch.bfloat16)
            x_bf = _uncast(x, torch.bfloat16)
            if _dtype_of(x) == torch.bfloat16:
                x_bf = x
            if _dtype_of(grad) == torch.bfloat16:
                g_bf = grad
            if g_bf is None or x_bf is None:
                # bf16 kernel doesn't apply — but the raw aten node can
                # still receive mixed fp32/bf16 args at RUNTIME once
                # resharding comm nodes (no meta) and fwd-side cast
                # folding detach runtime dtypes from the trace's; aten
                # hard-rejects that. Use the dtype-tolerant fp32
                # reference op and cast outputs back to the trace's
                # dtypes.
                with graph.inserting_before(n):
                    new = graph.call_function(
                        torch.ops.easydist_amd.ln_bwd_ref.default,
                        (grad, x, list(shape), mean, rstd, w, b,
                         list(mask)))
                _rewire_tuple(graph, n, new,
                              kernel_dtypes=[torch.float32, torch.float32,
                                             torch.float32])
                n_lowered += 1
                continue
            with graph.inserting_before(n):
                new = graph.call_function(
                    torch.ops.easydist_amd.layer_norm_bwd.default,
                    (g_bf, x_bf, mean, rstd, w, list(mask)))
            _rewire_tuple(graph, n, new,
                          kernel_dtypes=[torch.bfloat16, torch.float32,
                                         torch.float32])
            n_lowered += 1
    if n_lowered:
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: lowered %d layer_norm nodes", n_lowered)
    return n_lowered


def _sig(n):
    """(dtype, shape) of a node's tensor, or None when unknown. The dx
    getitem that lower_layer_norm creates carries no meta: it is the
    kernel's raw output, shaped and typed like the backward's x."""
    v = _val(n)
    if isinstance(v, torch.Tensor):
        return v.dtype, tuple(v.shape)
    if isinstance(n, fx.Node) and n.op == "call_function" \
            and n.target is operator.getitem and n.args[1] == 0 \
            and n.args[0].target in (
                torch.ops.easydist_amd.layer_norm_bwd.default,
                torch.ops.easydist_amd.layer_norm_bwd_res.default):
        return _sig(n.args[0].args[1])
    return None


def _plain_bf16_add(n) -> bool:
    """aten.add.Tensor of two equally shaped bf16 tensors, no alpha."""
    if not (n.op == "call_function" and n.target is aten.add.Tensor
            and len(n.args) == 2 and not n.kwargs
            and all(isinstance(a, fx.Node) for a in n.args)):
        return False
    so, sa, sb = _sig(n), _sig(n.args[0]), _sig(n.args[1])
    return so is not None and so[0] == torch.bfloat16 and so == sa == sb


def lower_norm_residual_fuse(gm: fx.GraphModule) -> int:
    """Fold the residual-stream adds into the LayerNorm kernels.

    Forward:   s = add(a, b); ln = layer_norm_fwd(s, w, b, eps)
            -> s, out, mean, rstd = add_layer_norm_fwd(a, b, w, b, eps)
               (every other user of s reads the fused op's first output)
    Backward:  d = add(g, getitem(layer_norm_bwd(...), 0)), either operand
               order, the dx feeding nothing else
            -> d, dw, db = layer_norm_bwd_res(..., res=g, mask)

    Both adds re-stream tensors the norm kernel already holds in registers;
    the fused ops give bit-identical results. Run AFTER lower_layer_norm.
    """
    graph = gm.graph
    ln_fwd = torch.ops.easydist_amd.layer_norm_fwd.default
    ln_bwd = torch.ops.easydist_amd.layer_norm_bwd.default
    add_ln_fwd = torch.ops.easydist_amd.add_layer_norm_fwd.default
    ln_bwd_res = torch.ops.easydist_amd.layer_norm_bwd_res.default
    n_fwd = n_bwd = 0

    for n in list(graph.nodes):
        if not _plain_bf16_add(n):
            continue
        ln = next((u for u in n.users if u.op == "call_function"
                   and u.target is ln_fwd and u.args[0] is n), None)
        if ln is None:
            continue
        with graph.inserting_before(n):
            fused = graph.call_function(add_ln_fwd,
                                        (n.args[0], n.args[1]) + ln.args[1:])
            s = graph.call_function(operator.getitem, (fused, 0))
        fused.meta = dict(ln.meta)
        s.meta = dict(n.meta)
        for u in list(ln.users):
            assert u.op == "call_function" and u.target is operator.getitem
            with graph.inserting_before(u):
                item = graph.call_function(operator.getitem,
                                           (fused, u.args[1] + 1))
            item.meta = dict(u.meta)
            u.replace_all_uses_with(item)
            graph.erase_node(u)
        graph.erase_node(ln)
        n.replace_all_uses_with(s)
        graph.erase_node(n)
        n_fwd += 1

    order = {node: i for i, node in enumerate(graph.nodes)}
    for n in list(graph.nodes):
        if not _plain_bf16_add(n):
            continue
        for g, dx in (n.args, n.args[::-1]):
            bwd = dx.args[0] if dx.op == "call_function" \
                and dx.target is operator.getitem and dx.args[1] == 0 \
                else None
            if bwd is None or bwd.op != "call_function" \
                    or bwd.target is not ln_bwd or len(dx.users) != 1:
                continue
            # the fused node takes the backward's place, where the dw/db
            # consumers expect it: g has to exist by then
            if order[g] > order[bwd]:
                continue
            with graph.inserting_before(bwd):
                fused = graph.call_function(
                    ln_bwd_res, bwd.args[:5] + (g, bwd.args[5]))
            fused.meta = dict(bwd.meta)
            order[fused] = order[bwd]
            for u in list(bwd.users):
                assert u.op == "call_function" \
                    and u.target is operator.getitem
                with graph.inserting_before(u):
                    item = graph.call_function(operator.getitem,
                                               (fused, u.args[1]))
                item.meta = dict(n.meta if u is dx else u.meta)
                order[item] = order[u]
                if u is dx:
                    n.replace_all_uses_with(item)
                    graph.erase_node(n)
                else:
                    u.replace_all_uses_with(item)
                graph.erase_node(u)
            graph.erase_node(bwd)
            n_bwd += 1
            break

    if n_fwd or n_bwd:
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: fused %d residual adds into LayerNorm "
                    "forwards, %d into backwards", n_fwd, n_bwd)
    return n_fwd + n_bwd


def _strip_t(n):
    """Return x if n is aten.t(x), else None."""
    if isinstance(n, fx.Node) and n.op == "call_function" \
            and n.target is aten.t.default:
        return n.args[0]
    return None


def _contig(n) -> bool:
    v = _val(n)
    return isinstance(v, torch.Tensor) and v.is_contiguous()


def lower_gemm(gm: fx.GraphModule) -> int:
    """Rewrite linear-layer matmuls to the hand-written MFMA GEMM ops.

    Post-sharding graph patterns (north-star requirement: every
    partitioned matmul on hand-written CDNA4 kernels; reference lowering
    shape: easydist/torch/passes/sharding.py:852+):

    * fwd:  addmm(bias, x, t(W)) / mm(x, t(W))      -> gemm_nt(x, W, bias)
    * dX:   mm(dY, t(t(W))) (W weight, contiguous)  -> gemm_nt(dY, W^T)
            with W^T materialized by ONE weight-sized transpose-copy —
            a few microseconds against a 100x bigger activation GEMM
    * dW:   mm(t(dY), X) (both reduce-dim-strided)  -> gemm_tn(dY, X)

    Only shapes inside the kernel envelope are rewritten; everything else
    stays on aten (hipBLASLt).  The ops themselves keep a per-shape
    profiled fallback (ops/gemm.py).
    """
    graph = gm.graph
    n_lowered = 0
    gemm_nt = torch.ops.easydist_amd.gemm_nt.default
    gemm_nn = torch.ops.easydist_amd.gemm_nn.default
    gemm_tn = torch.ops.easydist_amd.gemm_tn.default

    def bf16_2d(n):
        v = _val(n)
        return (isinstance(v, torch.Tensor) and v.dtype == torch.bfloat16
                and v.dim() == 2)

    def nt_ok(a_val, x_val):
        M, K = a_val.shape
        N, K2 = x_val.shape
        return K == K2 and K % 32 == 0 and N % 8 == 0 and M >= 16

    def tn_ok(x_val, b_val):
        R, P = x_val.shape
        R2, Q = b_val.shape
        return R == R2 and R % 32 == 0 and P % 128 == 0 and Q % 128 == 0

    for n in list(graph.nodes):
        if n.op != "call_function":
            continue
        if n.target is aten.addmm.default:
            bias, a, b = n.args[:3]
            if n.kwargs.get("alpha", 1) != 1 or n.kwargs.get("beta", 1) != 1:
                continue
        elif n.target is aten.mm.default:
            a, b = n.args
            bias = None
        else:
            continue
        if not (bf16_2d(a) and bf16_2d(b) and bf16_2d(n)):
            continue

        new = None
        x = _strip_t(b)
        if x is not None and _contig(x) and _contig(a):
            # NT: mm(a, t(x)) with x contiguous [N, K]
            if nt_ok(_val(a), _val(x)):
                with graph.inserting_before(n):
                    new = graph.call_function(gemm_nt, (a, x, bias))
        elif x is not None and _contig(a):
            y = _strip_t(x)
            if y is not None and _contig(y):
                # NN (dX = dY @ W): gemm_nn keeps the layout decision
                # inside the op — the hand route pays one weight-sized
                # transpose copy, the hipBLASLt route takes the strided
                # operand natively (the old graph-level clone(t(W))
                # charged BOTH routes)
                y_val = _val(y)
                if y_val is not None and y_val.shape[0] % 32 == 0 \
                        and y_val.shape[1] % 8 == 0 and _val(a).shape[0] >= 16:
                    # weight-size heuristic (both directions measured
                    # within one box): small weights -> the per-step
                    # clone is cheap and Tensile's NT layout beats its
                    # strided NN (legacy wins GPT-2 small by ~1%); big
                    # weights -> the clone dominates (gemm_nn wins
                    # GPT-2 1.3B by ~2%). Threshold 8M elements.
                    import os as _os
                    nn_env = _os.environ.get("EASYDIST_NN_LOWER", "auto")
                    use_nn = (nn_env == "1"
                              or (nn_env == "auto"
                                  and y_val.numel() >= (1 << 23)))
                    if use_nn:
                        with graph.inserting_before(n):
                            new = graph.call_function(gemm_nn, (a, y, bias))
                    else:
                        # legacy form: graph-level clone(t(W)) + gemm_nt
                        with graph.inserting_before(n):
                            yt = graph.call_function(aten.t.default, (y,))
                            ytc = graph.call_function(
                                aten.clone.default, (yt,),
                                {"memory_format": torch.contiguous_format})
                            new = graph.call_function(gemm_nt,
                                                      (a, ytc, bias))
                        try:
                            yt.meta["val"] = y_val.t()
                            ytc.meta["val"] = y_val.t().clone(
                                memory_format=torch.contiguous_format)
                        except Exception:
                            pass
        if new is None and bias is None:
            xa = _strip_t(a)
            if xa is not None and _contig(xa) and _contig(b) \
                    and tn_ok(_val(xa), _val(b)):
                # TN: mm(t(xa), b) -> gemm_tn(xa, b)
                with graph.inserting_before(n):
                    new = graph.call_function(gemm_tn, (xa, b))
        if new is None:
            continue
        new.meta = dict(n.meta)
        n.replace_all_uses_with(new)
        graph.erase_node(n)
        n_lowered += 1

    if n_lowered:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: lowered %d mm/addmm nodes to MFMA GEMM",
                    n_lowered)
    return n_lowered


def _rewire_tuple(graph: fx.Graph, old: fx.Node, new: fx.Node,
                  kernel_dtypes):
    """Point every getitem(old, k) at getitem(new, k). A consumer that is
    a cast TO the kernel's output dtype folds away; consumers expecting
    the old aten dtype get one explicit cast so semantics never change."""
    for u in list(old.users):
        if not (u.op == "call_function" and u.target is operator.getitem):
            continue
        k = u.args[1]
        with graph.inserting_before(u):
            item = graph.call_function(operator.getitem, (new, k))
        want = kernel_dtypes[k] if k < len(kernel_dtypes) else None
        old_dtype = _dtype_of(u)
        for uu in list(u.users):
            if uu.op == "call_function" and uu.target in CAST_OPS and \
                    _dtype_of(uu) == want:
                uu.replace_all_uses_with(item)
                graph.erase_node(uu)
        if list(u.users):
            if old_dtype is not None and want is not None \
                    and old_dtype != want:
                with graph.inserting_before(u):
                    cast = graph.call_function(
                        aten._to_copy.default, (item,),
                        {"dtype": old_dtype})
                u.replace_all_uses_with(cast)
            else:
                u.replace_all_uses_with(item)
        graph.erase_node(u)
    graph.erase_node(old)


# --------------------------------------------------------------------------
# SDPA + cross-entropy lowering for UNMODIFIED user models (reference
# capability: easydist README.md:14-36 / torch/api.py:227 — any plain
# PyTorch train step).  The builder's own models call the custom ops
# directly; a stock HF/torchvision model traces to the aten SDPA and
# log_softmax+nll nodes rewritten here.
# --------------------------------------------------------------------------
_SDPA_FWD = []
_SDPA_BWD = []
for _n in ("_scaled_dot_product_flash_attention",
           "_scaled_dot_product_flash_attention_for_cpu"):
    try:
        _SDPA_FWD.append(getattr(torch.ops.aten, _n).default)
        _SDPA_BWD.append(getattr(torch.ops.aten, _n + "_backward").default)
    except AttributeError:
        pass


def lower_sdpa(gm: fx.GraphModule) -> int:
    """aten flash-SDPA (fwd+bwd) -> easydist_amd::flash_attention(+bwd).

    Only the dropout-free, mask-free, default-scale form is rewritten
    (that is what inference/training transformers emit); the custom op
    itself falls back to exact aten math for shapes outside the HIP
    kernel envelope, so this rewrite never changes semantics.
    """
    graph = gm.graph
    n_lowered = 0
    flash = torch.ops.easydist_amd.flash_attention.default
    flash_bwd = torch.ops.easydist_amd.flash_attention_bwd.default

    for n in list(graph.nodes):
        if n.op != "call_function" or n.target not in _SDPA_FWD:
            continue
        q, k, v = n.args[:3]
        dropout_p = n.args[3] if len(n.args) > 3 else n.kwargs.get(
            "dropout_p", 0.0)
        causal = n.args[4] if len(n.args) > 4 else n.kwargs.get(
            "is_causal", False)
        if dropout_p not in (0, 0.0):
            continue
        if n.kwargs.get("attn_mask") is not None:
            continue
        if n.kwargs.get("scale") is not None:
            continue
        # locate consumers: out/lse getitems and the backward node
        out_gets, lse_gets, other = [], [], []
        bwd_nodes = []
        for u in list(n.users):
            if u.op == "call_function" and u.target is operator.getitem:
                idx = u.args[1]
                if idx == 0:
                    out_gets.append(u)
                elif idx == 1:
                    lse_gets.append(u)
                else:
                    other.append(u)
            else:
                other.append(u)
        ok = True
        for g in lse_gets + other:
            for uu in g.users:
                if not (uu.op == "call_function" and uu.target in _SDPA_BWD):
                    ok = False
        if not ok:
            continue
        for nn_ in graph.nodes:
            if nn_.op == "call_function" and nn_.target in _SDPA_BWD \
                    and nn_.args[1] is q and nn_.args[2] is k \
                    and nn_.args[3] is v:
                bwd_nodes.append(nn_)

        with graph.inserting_before(n):
            new = graph.call_function(flash, (q, k, v, bool(causal)))
            new_out = graph.call_function(operator.getitem, (new, 0))
            new_lse = graph.call_function(operator.getitem, (new, 1))
        qv = _val(q)
        if isinstance(qv, torch.Tensor):
            try:
                new_out.meta["val"] = qv.new_empty(tuple(qv.shape))
                new_lse.meta["val"] = qv.new_empty(tuple(qv.shape[:-1]),
                                                   dtype=torch.float32)
            except Exception:
                pass
        # the CPU SDPA variant returns [B,H,S,D] with [B,S,H,D]-layout
        # strides and downstream user code `view`s on them; our kernel
        # returns contiguous — restride when the original wasn't contig
        user_out = new_out
        ov = _val(out_gets[0]) if out_gets else None
        if isinstance(ov, torch.Tensor) and not ov.is_contiguous():
            with graph.inserting_before(n):
                t1 = graph.call_function(aten.transpose.int,
                                         (new_out, 1, 2))
                c1 = graph.call_function(
                    aten.clone.default, (t1,),
                    {"memory_format": torch.contiguous_format})
                user_out = graph.call_function(aten.transpose.int,
                                               (c1, 1, 2))
            if isinstance(qv, torch.Tensor):
                try:
                    t1.meta["val"] = qv.new_empty(tuple(qv.shape)) \
                        .transpose(1, 2)
                    c1.meta["val"] = t1.meta["val"].clone(
                        memory_format=torch.contiguous_format)
                    user_out.meta["val"] = c1.meta["val"].transpose(1, 2)
                except Exception:
                    pass
        for g in out_gets:
            g.replace_all_uses_with(user_out)
            graph.erase_node(g)
        for b in bwd_nodes:
            grad = b.args[0]
            with graph.inserting_before(b):
                nb = graph.call_function(
                    flash_bwd, (grad, q, k, v, new_out, new_lse,
                                bool(causal)))
            nb.meta = dict(b.meta)
            # dq/dk/dv getitems keep indices 0/1/2; restride like the
            # forward when the aten grads were non-contiguous views
            for u in list(b.users):
                if u.op == "call_function" and u.target is operator.getitem:
                    with graph.inserting_before(u):
                        item = graph.call_function(operator.getitem,
                                                   (nb, u.args[1]))
                    uv = _val(u)
                    res = item
                    if isinstance(uv, torch.Tensor) \
                            and not uv.is_contiguous():
                        with graph.inserting_before(u):
                            tt = graph.call_function(aten.transpose.int,
                                                     (item, 1, 2))
                            cc = graph.call_function(
                                aten.clone.default, (tt,),
                                {"memory_format": torch.contiguous_format})
                            res = graph.call_function(aten.transpose.int,
                                                      (cc, 1, 2))
                        try:
                            item.meta["val"] = uv.contiguous()
                            tt.meta["val"] = item.meta["val"].transpose(1, 2)
                            cc.meta["val"] = tt.meta["val"].clone(
                                memory_format=torch.contiguous_format)
                            res.meta["val"] = cc.meta["val"].transpose(1, 2)
                        except Exception:
                            pass
                    else:
                        item.meta = dict(u.meta)
                    u.replace_all_uses_with(res)
                    graph.erase_node(u)
            graph.erase_node(b)
        for g in lse_gets + other:
            graph.erase_node(g)
        graph.erase_node(n)
        n_lowered += 1

    if n_lowered:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: lowered %d SDPA nodes to flash_attention",
                    n_lowered)
    return n_lowered


def lower_cross_entropy(gm: fx.GraphModule) -> int:
    """log_softmax + nll_loss (fwd+bwd) -> fused CE kernels.

    Rewrites the whole diamond exactly, including ignore_index masking
    and mean/sum reduction, without ever materializing the [N, V]
    log-softmax (1.6 GB fp32 at GPT-2 shapes).
    """
    graph = gm.graph
    aten_ = torch.ops.aten
    ce_rows = torch.ops.easydist_amd.ce_fwd_rows.default
    ce_bwd = torch.ops.easydist_amd.ce_bwd.default
    n_lowered = 0

    for ls in list(graph.nodes):
        if ls.op != "call_function" \
                or ls.target is not aten_._log_softmax.default:
            continue
        x, dim, _h2f = ls.args
        xv = _val(x)
        if not (isinstance(xv, torch.Tensor) and xv.dim() == 2
                and dim in (-1, 1)):
            continue
        nll_f = nll_b = lsm_b = None
        ok = True
        for u in ls.users:
            if u.target is aten_.nll_loss_forward.default:
                nll_f = u
            elif u.target is aten_.nll_loss_backward.default:
                nll_b = u
            elif u.target is aten_._log_softmax_backward_data.default:
                lsm_b = u
            else:
                ok = False
        if not ok or nll_f is None:
            continue
        _, target, weight, reduction, ignore_index = nll_f.args[:5]
        if weight is not None or reduction not in (1, 2):
            continue
        if nll_b is not None and lsm_b is None:
            continue
        # the log_softmax_backward must consume the nll_backward's output
        if lsm_b is not None and nll_b is not None \
                and lsm_b.args[0] is not nll_b:
            continue

        with graph.inserting_before(nll_f):
            valid = graph.call_function(aten_.ne.Scalar,
                                        (target, ignore_index))
            zeros = graph.call_function(aten_.zeros_like.default, (target,))
            safe = graph.call_function(aten_.where.self,
                                       (valid, target, zeros))
            rows = graph.call_function(ce_rows, (x, safe))
            nll_rows = graph.call_function(operator.getitem, (rows, 0))
            lse = graph.call_function(operator.getitem, (rows, 1))
            validf = graph.call_function(aten_._to_copy.default, (valid,),
                                         {"dtype": torch.float32})
            masked = graph.call_function(aten_.mul.Tensor,
                                         (nll_rows, validf))
            loss_sum = graph.call_function(aten_.sum.default, (masked,))
            cnt = graph.call_function(aten_.sum.default, (validf,))
            if reduction == 1:      # mean over VALID rows
                loss = graph.call_function(aten_.div.Tensor,
                                           (loss_sum, cnt))
            else:                   # sum
                loss = loss_sum
        # rewire forward getitems: 0 -> loss, 1 -> total_weight (cnt)
        for u in list(nll_f.users):
            if u.op == "call_function" and u.target is operator.getitem:
                tgt = loss if u.args[1] == 0 else cnt
                u.replace_all_uses_with(tgt)
                graph.erase_node(u)
        # backward: dlogits = ce_bwd(per-row grads, x, safe, lse)
        if nll_b is not None and lsm_b is not None:
            gl = nll_b.args[0]
            with graph.inserting_before(lsm_b):
                g_rows = graph.call_function(aten_.mul.Tensor, (validf, gl))
                if reduction == 1:
                    g_rows = graph.call_function(aten_.div.Tensor,
                                                 (g_rows, cnt))
                dlogits = graph.call_function(ce_bwd,
                                              (g_rows, x, safe, lse))
            dlogits.meta = dict(lsm_b.meta)
            lsm_b.replace_all_uses_with(dlogits)
            graph.erase_node(lsm_b)
            graph.erase_node(nll_b)
        graph.erase_node(nll_f)
        graph.erase_node(ls)
        n_lowered += 1

    if n_lowered:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: lowered %d cross-entropy chains to fused CE",
                    n_lowered)
    return n_lowered


def _strip_view(n):
    if isinstance(n, fx.Node) and n.op == "call_function" \
            and n.target in (aten.view.default, aten._unsafe_view.default):
        return n.args[0]
    return None


def lower_gelu_bwd_fuse(gm: fx.GraphModule) -> int:
    """Fuse gelu_backward into the MFMA GEMM that produces its grad.

    Pattern (c_proj dX of a transformer MLP):
        g2 = gemm_nt(dY, Wt)            # the incoming gradient
        g3 = view(g2, [B,T,N])
        d  = gelu_backward(g3, x3)      # x3 = view(pre-act 2d)
    ->  g2' = gemm_nt_act(dY, Wt, None, GELU_BWD, x2); d := view(g2')
    The epilogue multiplies by dgelu(aux) during the (already coalesced)
    C store — removes one full activation-sized read+write pass.
    """
    graph = gm.graph
    nt_act = torch.ops.easydist_amd.gemm_nt_act.default
    nn_act = torch.ops.easydist_amd.gemm_nn_act.default
    nt = torch.ops.easydist_amd.gemm_nt.default
    nn = torch.ops.easydist_amd.gemm_nn.default
    n_fused = 0
    for n in list(graph.nodes):
        if n.op != "call_function" \
                or n.target is not aten.gelu_backward.default:
            continue
        approx = n.kwargs.get("approximate",
                              n.args[2] if len(n.args) > 2 else "none")
        act = 2 if approx == "tanh" else 4
        g, x = n.args[0], n.args[1]
        # strip 3-D views down to the 2-D gemm / pre-act nodes
        g2 = _strip_view(g) if _strip_view(g) is not None else g
        x2 = _strip_view(x) if _strip_view(x) is not None else x
        if not (isinstance(g2, fx.Node) and g2.op == "call_function"
                and g2.target in (nt, nn)):
            continue
        gv, xv = _val(g2), _val(x2)
        if not (isinstance(xv, torch.Tensor) and xv.dim() == 2
                and isinstance(gv, torch.Tensor)
                and tuple(xv.shape) == tuple(gv.shape)
                and xv.is_contiguous()):
            continue
        # the grad must not feed anything else (its value changes)
        g_users = set(g2.users) | (set(g.users) if g is not g2 else set())
        if g_users - {n, g}:
            continue
        a, bt, bias = g2.args
        fused_op = nt_act if g2.target is nt else nn_act
        with graph.inserting_before(g2):
            new = graph.call_function(fused_op, (a, bt, bias, act, x2))
        new.meta = dict(g2.meta)
        g2.replace_all_uses_with(new)
        graph.erase_node(g2)
        # gelu_backward output == the (now activated) gemm, viewed 3-D
        if g is not g2:
            n.replace_all_uses_with(g)
        else:
            n.replace_all_uses_with(new)
        graph.erase_node(n)
        n_fused += 1
    if n_fused:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: fused %d gelu_backward into GEMM epilogues",
                    n_fused)
    return n_fused


def lower_bias_grad_fuse(gm: fx.GraphModule) -> int:
    """Fuse the linear-bias gradient column sum into the dW TN GEMM.

    Pattern: sum(dY2, [0], keepdim) alongside gemm_tn(dY2, X) — the TN
    kernel already streams every element of dY through LDS; it
    accumulates the column sum there instead of aten re-reading the
    whole activation-sized gradient.
    """
    graph = gm.graph
    tn = torch.ops.easydist_amd.gemm_tn.default
    tn_asum = torch.ops.easydist_amd.gemm_tn_asum.default
    n_fused = 0
    for n in list(graph.nodes):
        if n.op != "call_function" or n.target is not tn:
            continue
        dy, xb = n.args
        sum_nodes = [u for u in dy.users
                     if u.op == "call_function"
                     and u.target is aten.sum.dim_IntList
                     and list(u.args[1]) == [0]
                     and u.kwargs.get("dtype") is None]
        if not sum_nodes:
            continue
        with graph.inserting_before(n):
            new = graph.call_function(tn_asum, (dy, xb))
            dw = graph.call_function(operator.getitem, (new, 0))
            asum = graph.call_function(operator.getitem, (new, 1))
        dw.meta = dict(n.meta)
        n.replace_all_uses_with(dw)
        graph.erase_node(n)
        for sn in sum_nodes:
            keepdim = len(sn.args) > 2 and sn.args[2]
            sv = _val(sn)
            with graph.inserting_before(sn):
                out = asum
                if isinstance(sv, torch.Tensor) and sv.dtype != torch.float32:
                    out = graph.call_function(aten._to_copy.default, (out,),
                                              {"dtype": sv.dtype})
                if keepdim:
                    # -1: the traced global length is wrong once the
                    # transform shards the bias grad
                    out = graph.call_function(aten.view.default,
                                              (out, [1, -1]))
            out.meta["val"] = sv
            sn.replace_all_uses_with(out)
            graph.erase_node(sn)
        n_fused += 1
    if n_fused:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: fused %d bias-grad sums into TN GEMMs",
                    n_fused)
    return n_fused


def lower_attn_pack(gm: fx.GraphModule) -> int:
    """Collapse the dq/dk/dv repack chain into a packed flash backward.

    The qkv projection's autograd materializes

        cat([unsafe_view(clone(transpose(flash_bwd[i], 1, 2)))
             for i in (0, 1, 2)], dim=2)

    — three strided [B,H,S,D]->[B,S,H*D] gathers plus a cat copy, ~1.2 GB
    of pure layout traffic per GPT layer at batch 64 (reference keeps the
    equivalent aten chain: easydist/torch/experimental/pp/split_utils.py
    has no such fusion). flash_attention_bwd_pack writes dq/dk/dv through
    output strides straight into one [B, S, 3*H*D] buffer, so the whole
    chain becomes one node. Run AFTER lower_sdpa. With grouped-query
    attention dk and dv are [B,Hkv,S,D], the cat is [B, S, (H+2*Hkv)*D]
    and the packed op lays its buffer out the same way: the match needs
    no head counts.
    """
    flash_bwd = torch.ops.easydist_amd.flash_attention_bwd.default
    flash_pack = torch.ops.easydist_amd.flash_attention_bwd_pack.default
    graph = gm.graph
    n_fused = 0

    def _single_user(n):
        return len(n.users) == 1

    for n in list(graph.nodes):
        if n.op != "call_function" or n.target is not aten.cat.default:
            continue
        parts = n.args[0]
        dim = n.args[1] if len(n.args) > 1 else 0
        if len(parts) != 3 or dim not in (2, -1):
            continue
        fab = None
        chains = []
        ok = True
        for want_idx, view in enumerate(parts):
            # view(...chain of (1,2)-transposes and clones...) — the model's
            # [B,H,S,D]->[B,S,H*D] repack, possibly with lower_sdpa's
            # stride-relayout (transpose+clone+transpose) in between. A NET
            # odd transpose count is the [B,S,...] layout the cat needs.
            chain = [view]
            m = view
            if m.op != "call_function" or m.target not in (
                    aten._unsafe_view.default, aten.view.default):
                ok = False
                break
            m = m.args[0]
            n_t = 0
            gi = None
            while True:
                if not isinstance(m, fx.Node) or not _single_user(m):
                    break
                if (m.target is aten.transpose.int
                        and set(m.args[1:]) == {1, 2}):
                    n_t += 1
                elif m.target is aten.clone.default:
                    pass
                elif m.target is operator.getitem:
                    gi = m
                    break
                else:
                    break
                chain.append(m)
                if len(chain) > 8:
                    break
                m = m.args[0]
            if gi is None or n_t % 2 == 0 or gi.args[1] != want_idx:
                ok = False
                break
            chain.append(gi)
            src = gi.args[0]
            if src.op != "call_function" or src.target is not flash_bwd:
                ok = False
                break
            if fab is None:
                fab = src
            elif fab is not src:
                ok = False
                break
            chains.append(chain)
        if not ok or fab is None:
            continue
        # every flash_bwd consumer must be one of the three getitems
        gitems = {c[-1] for c in chains}
        if set(fab.users) != gitems:
            continue
        # cat must be each view's only consumer (views feed nothing else)
        if any(len(v.users) != 1 for v in parts):
            continue
        with graph.inserting_before(fab):
            pack = graph.call_function(flash_pack, tuple(fab.args))
        pack.meta = dict(n.meta)
        n.replace_all_uses_with(pack)
        graph.erase_node(n)
        for chain in chains:
            for m in chain:
                graph.erase_node(m)
        graph.erase_node(fab)
        n_fused += 1

    if n_fused:
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: packed %d flash-bwd repack chains", n_fused)
    return n_fused


def lower_gelu_fwd_fuse(gm: fx.GraphModule) -> int:
    """Fuse the forward gelu into the MFMA GEMM that produces its input.

    Pattern (after lower_gemm):

        pre = gemm_nt(x2, w, bias)      # [M, N]
        v   = view(pre, [b, s, N])
        y   = gelu(v, approximate=...)

    becomes ``act2, pre = gemm_nt_gelu(x2, w, bias, tanh)`` with ``y``
    re-created as a view of ``act2``. The epilogue applies gelu during
    the (already coalesced) store pass and writes the pre-activation as a
    second output for gelu_backward, so the standalone activation kernel
    and its HBM re-read of the GEMM result disappear.
    """
    gemm_nt = torch.ops.easydist_amd.gemm_nt.default
    gemm_nt_gelu = torch.ops.easydist_amd.gemm_nt_gelu.default
    graph = gm.graph
    n_fused = 0
    for n in list(graph.nodes):
        if n.op != "call_function" or n.target is not aten.gelu.default:
            continue
        approx = "none"
        if len(n.args) > 1:
            approx = n.args[1]
        approx = n.kwargs.get("approximate", approx)
        v = n.args[0]
        views = (aten.view.default, aten._unsafe_view.default)
        if v.op == "call_function" and v.target in views:
            gnt = v.args[0]
            view_args = v.args[1]
        else:
            gnt = v
            view_args = None
        if gnt.op != "call_function" or gnt.target is not gemm_nt:
            continue
        with graph.inserting_before(gnt):
            fused = graph.call_function(
                gemm_nt_gelu, tuple(gnt.args) + (approx == "tanh",))
            act2 = graph.call_function(operator.getitem, (fused, 0))
            pre2 = graph.call_function(operator.getitem, (fused, 1))
        act2.meta = dict(gnt.meta)
        pre2.meta = dict(gnt.meta)
        gnt.replace_all_uses_with(pre2)
        if view_args is not None:
            with graph.inserting_before(n):
                act_v = graph.call_function(aten.view.default,
                                            (act2, view_args))
            act_v.meta = dict(n.meta)
            n.replace_all_uses_with(act_v)
        else:
            n.replace_all_uses_with(act2)
        graph.erase_node(n)
        graph.erase_node(gnt)
        n_fused += 1
    if n_fused:
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: fused %d forward gelu into GEMM epilogues",
                    n_fused)
    return n_fused


def _descendants(node: fx.Node) -> set:
    seen, stack = set(), [node]
    while stack:
        for u in stack.pop().users:
            if u not in seen:
                seen.add(u)
                stack.append(u)
    return seen


def lower_swiglu(gm: fx.GraphModule) -> int:
    """silu(a) * b and its autograd -> easydist_amd::swiglu(+_bwd).

    Forward:   mul(silu(a), b), either operand order, a and b of one shape
               and dtype (no broadcast, no cast in between)
            -> swiglu(a, b)
    Backward:  dup = mul(g, silu(a)); dgate = silu_backward(mul(g, b), a),
               the same g in both, either operand order
            -> dgate, dup = swiglu_bwd(g, a, b)

    The aten chain moves 5 activation-sized tensors forward and 9 backward
    and keeps silu(a) alive in between; the fused kernels move 3 and 5 and
    recompute the sigmoid from a. A forward without a matching backward
    (an inference graph) still fuses; a backward whose pieces do not all
    match is left alone, and so is any mul of the silu with a value derived
    from it. In fp32 and fp64 the ops run the very aten calls they replace,
    so the rewrite changes no bit there. Returns forward + backward fusions.
    """
    graph = gm.graph
    swiglu = torch.ops.easydist_amd.swiglu.default
    swiglu_bwd = torch.ops.easydist_amd.swiglu_bwd.default
    n_fwd = n_bwd = 0

    def same(*nodes):
        """One shape and dtype on every node's val."""
        vals = [_val(x) for x in nodes]
        return all(isinstance(v, torch.Tensor) for v in vals) \
            and all(v.shape == vals[0].shape and v.dtype == vals[0].dtype
                    for v in vals)

    def contig(*nodes):
        """Laid out as the ops' outputs are: new contiguous tensors."""
        return all(_val(x).is_contiguous() for x in nodes)

    def is_mul(m):
        """mul.Tensor of two different nodes."""
        return isinstance(m, fx.Node) and m.op == "call_function" \
            and m.target is aten.mul.Tensor and len(m.args) == 2 \
            and not m.kwargs \
            and all(isinstance(a, fx.Node) for a in m.args) \
            and m.args[0] is not m.args[1]

    def mul_other(m, x):
        """The other operand of m = mul.Tensor(x, y) / (y, x), or None."""
        if is_mul(m) and x in m.args:
            return m.args[1] if m.args[0] is x else m.args[0]
        return None

    def fuse_fwd(n, a, b):
        with graph.inserting_before(n):
            fused = graph.call_function(swiglu, (a, b))
        fused.meta = dict(n.meta)
        order[fused] = order[n]
        n.replace_all_uses_with(fused)
        graph.erase_node(n)

    order = {x: i for i, x in enumerate(graph.nodes)}
    for sl in list(graph.nodes):
        if sl.op != "call_function" or sl.target is not aten.silu.default:
            continue
        a = sl.args[0]
        if not isinstance(a, fx.Node):
            continue
        # a product of the silu with something computed from it is never
        # the activation: a gradient reaches back here through the loss
        desc = _descendants(sl)
        muls = {}         # the other operand -> mul(silu, other)
        for n in sorted(sl.users, key=order.__getitem__):
            other = mul_other(n, sl)
            if other is not None and other not in muls:
                muls[other] = n
        taken = set()

        # the triples first. silu_backward(mul(x, y), a) with mul(silu, x)
        # and mul(silu, y) both there: one of x, y is the up operand and
        # the other the gradient, and the activation is the product that
        # the trace computed first.
        for sb in list(a.users):
            if sb.op != "call_function" or len(sb.args) != 2 \
                    or sb.target is not aten.silu_backward.default \
                    or sb.args[1] is not a:
                continue
            if not is_mul(sb.args[0]):
                continue
            x, y = sb.args[0].args
            fwd, m1 = muls.get(x), muls.get(y)
            if fwd is None or m1 is None or {fwd, m1} & taken:
                continue
            b, g = x, y
            if order[m1] < order[fwd]:
                fwd, m1, b, g = m1, fwd, y, x
            if b in desc or not same(a, b, g, sl, fwd, m1, sb) \
                    or not contig(fwd, m1, sb):
                continue
            # the fused node goes where the first of the two stood: its
            # operands have to exist by then
            first = m1 if order[m1] < order[sb] else sb
            if order[g] > order[first] or order[b] > order[first]:
                continue
            fuse_fwd(fwd, a, b)
            with graph.inserting_before(first):
                bwd = graph.call_function(swiglu_bwd, (g, a, b))
                dgate = graph.call_function(operator.getitem, (bwd, 0))
                dup = graph.call_function(operator.getitem, (bwd, 1))
            bwd.meta = dict(sb.meta)
            bwd.meta["val"] = (_val(sb), _val(m1))
            dgate.meta = dict(sb.meta)
            dup.meta = dict(m1.meta)
            order[bwd] = order[dgate] = order[dup] = order[first]
            sb.replace_all_uses_with(dgate)
            m1.replace_all_uses_with(dup)
            graph.erase_node(sb)
            graph.erase_node(m1)
            taken.update((fwd, m1))
            n_fwd += 1
            n_bwd += 1

        # a forward with no backward of this form (an inference graph)
        for b, n in muls.items():
            if n in taken or b in desc:
                continue
            if same(a, b, sl, n) and contig(n):
                fuse_fwd(n, a, b)
                n_fwd += 1

    if n_fwd or n_bwd:
        # the silu and the mul(g, b) that fed silu_backward die here: that
        # is how the saved activation disappears
        graph.eliminate_dead_code()
        graph.lint()
        gm.recompile()
        logger.info("lower_hip: fused %d silu*mul into swiglu, %d backward "
                    "triples into swiglu_bwd", n_fwd, n_bwd)
    return n_fwd + n_bwd
