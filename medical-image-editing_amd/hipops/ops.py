"""Differentiable operators over the C ABI of libvqwnet_hip.so.

Every function takes / returns torch tensors that live on a ROCm device; PyTorch is
used only for device memory (caching allocator), the current stream and the
autograd tape.  All arithmetic happens in the hand-written HIP kernels; a missing
library or a CPU tensor raises (no eager fallback).

4-D activations are logically NCHW and physically NHWC (torch.channels_last).
Conv weights are logically OIHW and physically OHWI (channels_last too).
"""
import contextlib
import ctypes
import math
import os

import torch
import torch.distributed as dist

from . import _lib
from .library import Dispatch as _D

CL = torch.channels_last


# Kernels are reached through the PyTorch dispatcher: every entry point of the C ABI is an operator torch.ops.vqw.<name>
# with a schema derived from its prototype (hipops/library.py; mutation annotations from the `const` qualifiers).
_dispatch = None


def _L():
    global _dispatch
    if _dispatch is None:
        _dispatch = _D()
    return _dispatch


def _raw(t):
    """Raw device pointer for the few host-side entry points that take pointer arrays by value."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _raw_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("hipops operators need tensors on a ROCm device (got %s); "
                               "there is no CPU fallback" % t.device)


def nhwc(x):
    """Dense fp32 NHWC view of a 4-D tensor (no copy when it already is)."""
    if x.dtype != torch.float32:
        raise RuntimeError("hipops operators are fp32 (got %s)" % x.dtype)
    if x.dim() != 4:
        raise RuntimeError("expected a 4-D (N,C,H,W) tensor, got shape %s" % (tuple(x.shape),))
    if not x.is_contiguous(memory_format=CL):
        x = x.contiguous(memory_format=CL)
    # size-1 dims make PyTorch's stride check ambiguous; normalise the strides we rely on
    N, C, H, W = x.shape
    if x.stride() != (H * W * C, 1, W * C, C):
        x = x.as_strided((N, C, H, W), (H * W * C, 1, W * C, C))
    return x


def empty_nhwc(N, C, H, W, like):
    return torch.empty((N, C, H, W), dtype=torch.float32, device=like.device, memory_format=CL)


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def _mean_rstd(x, part, eps):
    """(mean, rstd) per (image, channel) of the NHWC tensor x, [N * C * 2] floats: from the statistics partials `part` that the
    convolution which produced x left in its epilogue when given, else by a reduction pass over x."""
    N, C, H, W = x.shape
    L = _L()
    mr = torch.empty(N * C * 2, dtype=torch.float32, device=x.device)
    if part is not None:
        L.vqw_inorm_stats_parts(part, part.numel() // (N * C * 2), mr, N, H * W, C, eps)
    else:
        ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
        L.vqw_inorm_stats(x, mr, ws, ws.numel(), N, H * W, C, eps)
    return mr


def _inorm_fwd(x, y, y_cstride, y_coff, part, eps, relu):
    """InstanceNorm(+ReLU) of x into the channels [y_coff, y_coff + C) of y (statistics as in _mean_rstd); returns (mean, rstd)."""
    N, C, H, W = x.shape
    L = _L()
    mr = torch.empty(N * C * 2, dtype=torch.float32, device=x.device)
    if part is not None:
        L.vqw_inorm_fwd_parts(x, y, y_cstride, y_coff, mr, part, part.numel() // (N * C * 2), N, H * W, C, eps, int(relu))
    else:
        ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
        L.vqw_inorm_fwd(x, y, y_cstride, y_coff, mr, ws, ws.numel(), N, H * W, C, eps, int(relu))
    return mr


def _inorm_bwd(x, mr, gy, relu, gy_cstride=None, gy_coff=0):
    """Gradient of InstanceNorm(+ReLU) at its raw input x; gy_cstride / gy_coff: where x's channels sit in a wider gy."""
    N, C, H, W = x.shape
    L = _L()
    gx = torch.empty_like(x, memory_format=CL)
    ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
    L.vqw_inorm_bwd(x, mr, gy, C if gy_cstride is None else gy_cstride, gy_coff, gx, ws, ws.numel(), N, H * W, C, int(relu))
    return gx


def _flat(t):
    if t.dtype != torch.float32:
        raise RuntimeError("expected fp32")
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------
# weight-gradient side stream
# ----------------------------------------------------------------------------------------------
# In backward the weight gradient of a conv is a leaf of the dependency chain: nothing downstream needs it before the
# optimiser.  It is therefore enqueued on a side HIP stream, where the MFMA-bound wgrad kernels overlap with the
# HBM-bound normalisation / element-wise backward kernels of the main chain, and written straight into `param.grad`
# (overwrite on the first use of a step, in-kernel accumulate afterwards — both views of a step share one buffer, no
# autograd add pass).  The main stream re-joins the side stream at the end of the backward pass (engine callback).
# VQW_WGRAD_STREAM=0 disables it (weight gradients then flow through autograd as usual).
WGRAD_ASYNC = os.environ.get("VQW_WGRAD_STREAM", "1") != "0"
_side_streams = {}
_join_queued_for = None        # id of the backward pass (autograd graph task) whose end-of-pass lane join is queued
grad_ready_listeners = []      # callables(param): the param's gradient is final and enqueued on the side stream


# The DDP detection below reads a private class attribute of torch.  On a torch build without it the check would silently
# say "no DDP" and the reducer would never see the conv weight gradients (hang or unsynchronised training), so its absence
# switches the out-of-band route off for good instead: every weight gradient then flows through autograd, which is always
# correct.  set_wgrad_route("autograd") is the explicit form a wrapper can call.
_DDP = torch.nn.parallel.DistributedDataParallel
_WGRAD_ROUTE = "auto" if hasattr(_DDP, "_active_ddp_module") else "autograd"


def set_wgrad_route(route):
    """"auto": conv weight gradients of leaf parameters are written out-of-band on the side stream unless a DDP forward is
    active or the parameter carries foreign hooks; "autograd": always through autograd.  Returns the previous route."""
    global _WGRAD_ROUTE
    if route not in ("auto", "autograd"):
        raise ValueError("wgrad route must be 'auto' or 'autograd'")
    old, _WGRAD_ROUTE = _WGRAD_ROUTE, route
    return old


def wgrad_through_autograd(*params):
    """True when weight gradients must flow through autograd instead of being written out-of-band on a side stream:
    inside a torch DistributedDataParallel forward (its reducer learns about a gradient from the AccumulateGrad hook of
    the parameter; the reference launches under Lightning's DDPPlugin, run_vqwnet.py:112-121) or when somebody
    registered a hook on the parameter."""
    if _WGRAD_ROUTE == "autograd" or getattr(_DDP, "_active_ddp_module", None) is not None:
        return True
    for p in params:
        if p is None:
            continue
        # (the data-parallel reducer of this package listens on both routes and marks its own hooks)
        if p._backward_hooks or len(getattr(p, "_post_accumulate_grad_hooks", None) or ()) > p.__dict__.get("_vqw_own_hooks", 0):
            return True
    return False


def _order_begin(token):
    """In-place updates of a module buffer (BN running stats, VQ codebook) keep host program order even when the two
    views of a step run on different streams: wait for the event the previous updater left on the buffer."""
    prev = token.__dict__.get("_vqw_order")
    cur = torch.cuda.current_stream()
    if prev is not None and prev[1] != cur:
        cur.wait_event(prev[0])
    return cur


def _order_end(token, cur):
    token.__dict__["_vqw_order"] = (cur.record_event(), cur)


def reset_pending(params):
    """Forget forward passes that were never back-propagated (call before the forwards of a training step)."""
    for p in params:
        if hasattr(p, "_vqw_pending"):
            p._vqw_pending = 0


# Weight gradients alternate between WGRAD_LANES side streams (a parameter keeps its lane: the second view accumulates
# into the first view's result).  One layer's slab reduction (a short, latency-bound launch that depends on the layer's
# wgrad kernel) then overlaps the next layer's wgrad kernel; on a single stream those gaps were exposed, most of all
# in the last tenth of the step when only weight gradients are left to run.  A gradient-ready listener that reads
# gradients of several parameters (data parallel: a bucket is flattened on the lane that announces its last gradient)
# orders its lane after the others first: sync_wgrad_lanes().
WGRAD_LANES = 2        # (one lane and three lanes measured slower: DESIGN §5)
_lane_counter = 0


def wgrad_stream(device, lane=0):
    dev = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (dev, lane)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=dev)
        _side_streams[key] = st
    return st


def sync_wgrad_lanes():
    """Order the current stream after everything enqueued so far on the weight-gradient lanes."""
    if not _side_streams:
        return
    cur = torch.cuda.current_stream()
    for st in _side_streams.values():
        if st.device == cur.device and st != cur:
            cur.wait_stream(st)


def _wgrad_lane(param):
    global _lane_counter
    if WGRAD_LANES == 1:
        return 0
    lane = param.__dict__.get("_vqw_lane")
    if lane is None:
        lane = param.__dict__["_vqw_lane"] = _lane_counter % WGRAD_LANES
        _lane_counter += 1
    return lane


def _pass_id():
    """Identity of the running backward pass (autograd graph task); -1 outside of one."""
    return torch._C._current_graph_task_id()


def _join_side_stream():
    """Order the current stream after the weight-gradient lanes (idempotent), then fold the split-K slabs the lanes' weight
    gradient kernels have left (one launch for the whole pass, see _fold_flush)."""
    global _join_queued_for
    _join_queued_for = None
    for st in _side_streams.values():
        torch.cuda.current_stream(st.device).wait_stream(st)
    _fold_flush()


# Deferred slab folds (VQW_FOLD_DEFER=0: every weight-gradient call folds its own slabs, two short launches per layer).
# A weight-gradient kernel leaves split-K slabs; folding them is a short, dependent launch behind every one of the ~110
# weight-gradient kernels of a step (dW and dbias: ~250 launches).  On the lanes the library only records the folds
# (vqw_fold_defer) and the end-of-pass lane join folds them all in ONE launch; the two views' folds into one gradient are
# summed in recording order (overwrite, then accumulate) - the same values in a fixed order.  The slab buffers are kept alive
# here until that launch is enqueued.  Off while a gradient-ready listener is registered (the overlapped data-parallel
# schedule needs a parameter's gradient final when it is announced).
FOLD_DEFER = os.environ.get("VQW_FOLD_DEFER", "1") != "0"
_fold_keep = []                # slab workspaces of the recorded folds
_fold_slots = []               # ring of [pinned host table, device table, event of the launch that read them]
_fold_next = 0
fold_flushes = 0               # batched fold launches since import (tests)


def _fold_active():
    return FOLD_DEFER and not grad_ready_listeners


def _fold_flush():
    """Fold every recorded slab set in one launch on the current stream (which the caller has ordered after the lanes)."""
    global _fold_next, fold_flushes
    lib = _lib.load()
    if not _fold_keep and lib.vqw_fold_pending() == 0:
        return
    need = int(lib.vqw_fold_table_bytes())
    cur = torch.cuda.current_stream()
    if len(_fold_slots) < 4:
        _fold_slots.append(None)
        _fold_next = len(_fold_slots) - 1
    slot = _fold_slots[_fold_next]
    if slot is not None:
        slot[2].synchronize()          # the launch that read this slot's tables has run (only ever waits when > 4 passes are in flight)
    if slot is None or slot[0].numel() < need or slot[1].device != cur.device:
        size = max(need, 1 << 16)
        slot = [torch.empty(size, dtype=torch.uint8, pin_memory=True), torch.empty(size, dtype=torch.uint8, device=cur.device), None]
    _lib.check(lib.vqw_fold_flush_host(ctypes.c_void_p(slot[0].data_ptr()), ctypes.c_void_p(slot[1].data_ptr()), slot[0].numel(),
                                       ctypes.c_void_p(cur.cuda_stream)), "vqw_fold_flush_host")
    slot[2] = cur.record_event()
    _fold_slots[_fold_next] = slot
    _fold_next = (_fold_next + 1) % 4
    fold_flushes += 1
    # the slab buffers belong to the lanes' memory pools: order the lanes after this launch before the pools may reuse them
    for st in _side_streams.values():
        if st.device == cur.device:
            st.wait_event(slot[2])
    _fold_keep.clear()


def _queue_lane_join():
    """Queue the lane join as an end-of-pass callback, once per backward pass.  The flag holds the pass's id, not a bool: a
    pass that ended in an exception (the engine skips every callback queued behind one that raises) cannot latch it."""
    global _join_queued_for
    tid = _pass_id()
    if _join_queued_for != tid:
        _join_queued_for = tid
        torch.autograd.Variable._execution_engine.queue_callback(_join_side_stream)


def join_streams():
    """End of a trainer step (begin_step() ... join_streams()): the BatchNorm counters deferred since begin_step() are bumped."""
    global _defer_counters
    _defer_counters = False
    flush_counters()


# Derived weight layouts (dgrad-packed, tap-collapsed) are cached on the parameter until it changes: both views of a
# step reuse them.  A parameter "changes" when torch bumps its version counter or when hipops.Adam (which updates
# through raw pointers) advances the epoch below.
_weight_epoch = 0


def bump_weight_epoch():
    global _weight_epoch
    _weight_epoch += 1


def _cached(weight, key, build, deps=()):
    """`deps`: further tensors the derived value is built from (concatenated convs)."""
    cache = weight.__dict__.setdefault("_vqw_cache", {})
    tag = (weight._version, _weight_epoch, weight.data_ptr()) + tuple((d._version, d.data_ptr()) for d in deps)
    cur = torch.cuda.current_stream()
    hit = cache.get(key)
    if hit is not None and hit[0] == tag:
        if hit[3] != cur:            # built on another stream (the other view): order this stream after the build
            cur.wait_event(hit[2])
        return hit[1]
    val = build()
    cache[key] = (tag, val, cur.record_event(), cur)
    return val


def _run_wgrad(L, x0, x1, gy, gw, gb, up0, ks, dilation, N, H, W, Cout, acc, collapsed, defer_fold=False):
    """dW / db on the CURRENT stream; `collapsed` selects the low-resolution form for 3x3-over-upsampled layers.
    defer_fold: the slab folds are only recorded (the caller has queued the end-of-pass lane join, which runs them)."""
    C0 = x0.shape[1]
    C1 = 0 if x1 is None else x1.shape[1]
    lib = _lib.load()
    defer_fold = defer_fold and _fold_active()
    for attempt in (0, 1):
        old = lib.vqw_fold_defer(1) if defer_fold else 0
        try:
            if collapsed and L.vqw_conv3x3_up2_wgrad_supported(C0, Cout, N, H // 2, W // 2):
                ws = _ws(L.vqw_conv3x3_up2_wgrad_ws_bytes(C0, Cout, N, H // 2, W // 2), gy)
                L.vqw_conv3x3_up2_wgrad(x0, gy, gw, gb, ws, ws.numel(), N, H // 2, W // 2, C0, Cout, int(acc))
            else:
                ws = _ws(L.vqw_conv2d_wgrad_ws_bytes(C0, C1, N, H, W, Cout, ks), gy)
                L.vqw_conv2d_wgrad(x0, C0, int(up0), x1, C1, gy, gw, gb, ws, ws.numel(), N, H, W, Cout, ks, dilation,
                                   int(acc))
        except RuntimeError as e:
            if defer_fold and attempt == 0 and "flush first" in str(e):
                # a third use of one weight inside a pass: fold what is recorded (on this lane, after the other lanes), retry
                lib.vqw_fold_defer(old)
                sync_wgrad_lanes()
                _fold_flush()
                continue
            raise
        finally:
            if defer_fold:
                lib.vqw_fold_defer(old)
        break
    if defer_fold:
        _fold_keep.append(ws)


def _out_of_band(needed, params, dense):
    """Whether the weight and bias gradients of one layer go out-of-band to the side lanes (_side_lane) instead of through
    autograd: `params` = (weight, bias) or, for a concatenated layer, (wa, ba, wb, bb), all of which must qualify; `needed`:
    autograd wants them; `dense`: the weights are in the layout the kernels write.  A yes registers a pending use on
    params[0], which the side lane counts down."""
    defer = bool(WGRAD_ASYNC and needed and all(p.is_leaf for p in params if p is not None) and not wgrad_through_autograd(*params)
                 and dense and all(b is None or b.is_contiguous() for b in params[1::2]))
    if defer:
        params[0]._vqw_pending = getattr(params[0], "_vqw_pending", 0) + 1
    return defer


@contextlib.contextmanager
def _side_lane(owner, tensors, announce):
    """Body runs on the weight-gradient lane of `owner`, ordered after what the current stream has enqueued; `tensors` are
    read there.  On the owner's last pending use the gradients of `announce` are final: every gradient-ready listener hears
    of them in that order.  The end-of-pass lane join is queued."""
    main = torch.cuda.current_stream()
    side = wgrad_stream(tensors[-1].device, _wgrad_lane(owner))
    ev = main.record_event()
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    with torch.cuda.stream(side):
        side.wait_event(ev)
        yield
        owner._vqw_pending = getattr(owner, "_vqw_pending", 1) - 1
        if owner._vqw_pending <= 0:
            owner._vqw_pending = 0
            for fn in grad_ready_listeners:
                for p in announce:
                    fn(p)
    _queue_lane_join()


def _deferred_wgrad(weight, bias, x0, x1, gy, up0, ks, dilation, N, H, W, Cout, collapsed=False):
    """Enqueue dW (and db) on the side stream, writing into weight.grad / bias.grad."""
    L = _L()
    C0 = x0.shape[1]
    C1 = 0 if x1 is None else x1.shape[1]
    with _side_lane(weight, (x0, x1, gy), (weight,) if bias is None else (weight, bias)):
        acc = weight.grad is not None
        if not acc:
            # (the parameter's own strides: channels_last for a 3 x 3 weight, the default ones for a 1 x 1 weight - the same memory order)
            weight.grad = torch.empty_strided((Cout, C0 + C1, ks, ks), weight.stride(), dtype=torch.float32, device=gy.device)
            if bias is not None:
                bias.grad = torch.empty(Cout, dtype=torch.float32, device=gy.device)
        gw, gb = weight.grad, (bias.grad if bias is not None else None)
        if gw.stride() != weight.stride():
            raise RuntimeError("conv2d: existing weight.grad layout does not match the parameter layout")
        _run_wgrad(L, x0, x1, gy, gw, gb, up0, ks, dilation, N, H, W, Cout, acc, collapsed, defer_fold=True)


# ----------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------
def _wino_weights(L, w_ohwi, Cin, Cout):
    """U = G w G^T [16][Cout][Cin] of a 3x3 layer (vqw_conv3x3_wino_prepare) in a fresh buffer."""
    buf = _ws(L.vqw_conv3x3_wino_ws_bytes(Cin, Cout), w_ohwi)
    L.vqw_conv3x3_wino_prepare(w_ohwi, buf, buf.numel(), Cin, Cout)
    return buf


def _wino_weights_dgrad(L, w_ohwi, Cin, Cout):
    """U of a 3x3 layer's INPUT-GRADIENT convolution (Cin = the layer's couts, Cout = its input channels), straight from the
    layer's weight: what _wino_weights gives on the packed input-gradient weights, without the pack launch."""
    buf = _ws(L.vqw_conv3x3_wino_ws_bytes(Cin, Cout), w_ohwi)
    L.vqw_conv3x3_wino_prepare_dgrad(w_ohwi, buf, buf.numel(), Cin, Cout)
    return buf


def _up2_weights(L, w_ohwi, Cin, Cout):
    """The collapsed weights of a 3x3 layer over a nearest x2 up-sampled input (vqw_conv3x3_up2_prepare) in a fresh buffer."""
    buf = _ws(L.vqw_conv3x3_up2_ws_bytes(Cin, Cout), w_ohwi)
    L.vqw_conv3x3_up2_prepare(w_ohwi, buf, buf.numel(), Cin, Cout)
    return buf


def _concat_layers(wa, ba, wb, bb, prepare=None):
    """(w, b) of the layers a and b concatenated along the output channels: w channels_last, or prepare(w) when the caller
    wants a derived layout of it; b None unless both layers have a bias."""
    Ca, Cin, ks, _ = wa.shape
    w = torch.empty((Ca + wb.shape[0], Cin, ks, ks), dtype=torch.float32, device=wa.device, memory_format=CL)
    w[:Ca].copy_(wa.detach())
    w[Ca:].copy_(wb.detach())
    if prepare is not None:
        w = prepare(w)
    b = torch.cat([ba.detach().reshape(-1), bb.detach().reshape(-1)]) if ba is not None and bb is not None else None
    return w, b


# Winograd F(2x2, 3x3) form of plain 3x3 layers.  The INPUT and WEIGHT GRADIENTS take it whenever the library serves the
# shape: they are linear in dy given the forward's masks, so the form's rounding difference (a few ulps of the accumulated
# magnitude) reaches the parameter gradients unamplified.  The training
# FORWARD does not by default: the Winograd form computes the four pixels of a tile by four different formulas, so equal
# inputs no longer give bit-equal outputs, and behind the quantised (piecewise constant) map the reference's max-pools sit
# on exact ties - on the config-4 step fixture the broken ties moved decoder gradients 3-5x the reference's own fp32 spread
# away from its fp64 gradient.  VQW_WINOGRAD_FWD=1 opts in (throughput runs).
WINOGRAD_FWD = os.environ.get("VQW_WINOGRAD_FWD", "0") == "1"
# Forward-only uses (torch.no_grad(): validation forward, run_recon) have no gradient to disturb and take the Winograd
# forward by themselves (VQW_WINOGRAD_EVAL=0: direct form there too).
WINOGRAD_EVAL = os.environ.get("VQW_WINOGRAD_EVAL", "1") != "0"
_in_custom_op = False          # set by hipops.functional around its no_grad() calls: those are training forwards

_wino_fwd_scope = 0            # > 0 inside `with winograd_forward():`


class winograd_forward:
    """Context: plain 3x3 layers called inside take the Winograd forward also in training.  For sub-networks in which nothing
    compares activations of different pixels (the decoder past its last max-pool).  The Winograd form computes the four pixels
    of a 2x2 tile by four different formulas, so mathematically equal outputs are no longer bit-equal; behind the quantised
    (piecewise constant) map the reference's max-pools sit on exact ties and a broken tie re-routes gradients."""

    def __enter__(self):
        global _wino_fwd_scope
        _wino_fwd_scope += 1

    def __exit__(self, *exc):
        global _wino_fwd_scope
        _wino_fwd_scope -= 1


def _decide_wino_fwd():
    """The per-call decision, handed to the autograd Functions as an explicit (non-differentiable) argument: a caller that
    reaches them without the wrapper, or a second host thread, cannot inherit another call's decision."""
    return bool(WINOGRAD_FWD or _wino_fwd_scope > 0 or (WINOGRAD_EVAL and not torch.is_grad_enabled() and not _in_custom_op))


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, weight, bias, dilation, up0, relu, want_stats=False, wino_fwd=False, grad_group=None, in_src=None):
        _dev(x0, x1, weight, bias)
        ctx.in_src = None
        if in_src is not None and x1 is None and not up0 and grad_group is None and dilation == 1 and weight.shape[2] == 3 \
                and ctx.needs_input_grad[0] and tuple(in_src[0].shape) == tuple(x0.shape) \
                and _L().vqw_conv3x3_wino_fwd_inbwd_parts(weight.shape[0], weight.shape[1], x0.shape[0], x0.shape[2], x0.shape[3]) > 0:
            ctx.in_src = in_src            # (raw input of the InstanceNorm whose output x0 is, its (mean, rstd), its ReLU flag)
        x0 = nhwc(x0)
        x1 = nhwc(x1) if x1 is not None else None
        w = nhwc(weight)
        Cout, Cin, ks, _ = weight.shape
        if w is not weight and ks == 1 and weight.is_contiguous() and w.data_ptr() == weight.data_ptr():
            # a 1 x 1 weight is dense in both memory formats and keeps the default strides: nhwc() re-strides the same memory.  The
            # parameter itself serves (the kernels take pointers): its derived layouts stay cached on it from step to step and its
            # gradient takes the side-lane route like every other layer's
            w = weight
        N = x0.shape[0]
        H, W = (x0.shape[2] * 2, x0.shape[3] * 2) if up0 else (x0.shape[2], x0.shape[3])
        c1 = 0 if x1 is None else x1.shape[1]
        if x0.shape[1] + c1 != Cin:
            raise RuntimeError("conv2d: input channels %d+%d do not match weight %s" % (x0.shape[1], c1, tuple(weight.shape)))
        if x1 is not None and (x1.shape[0] != N or x1.shape[2] != H or x1.shape[3] != W):
            raise RuntimeError("conv2d: concat source shape %s does not match %s" % (tuple(x1.shape), (N, c1, H, W)))
        if bias is not None:
            bias = _flat(bias)
        L = _L()
        h, wl = H // 2, W // 2
        up_ws = None
        stats = want_stats and not relu
        if up0 and x1 is None and ks == 3 and dilation == 1 and L.vqw_conv3x3_up2_supported(Cin, Cout, N, h, wl):
            # 3x3 over a nearest x2 up-sampled single source: collapsed onto the low-res grid (4/9 of the FLOPs)
            form = "up2"
            up_ws = _cached(weight, "up2", lambda: _up2_weights(L, w, Cin, Cout))
        elif wino_fwd and not up0 and x1 is None and ks == 3 and dilation == 1 and \
                L.vqw_conv3x3_wino_supported(Cin, Cout, N, H, W) and \
                (not stats or L.vqw_conv3x3_wino_fwd_stats_parts(Cin, Cout, N, H, W) > 0
                 or L.vqw_conv2d_fwd_stats_parts(Cin, 0, 0, N, H, W, Cout, ks, dilation) == 0):
            # (wanted statistics that only the direct form can leave for this height keep the direct form)
            # plain 3x3 layer: Winograd F(2x2, 3x3), 4/9 of the matrix work; U = G w G^T is kept while w is unchanged
            form = "wino"
        elif wino_fwd and not up0 and x1 is None and ks == 3 and dilation == 2 and \
                L.vqw_conv3x3_wino_dil2_supported(Cin, Cout, N, H, W) and \
                (not stats or L.vqw_conv3x3_wino_dil2_stats_parts(Cin, Cout, N, H, W) > 0):
            # dilation 2: the plain Winograd kernel on the four phase images of the tensors (same U as the plain layer)
            form = "dil2"
        else:
            form = "direct"
        if form in ("wino", "dil2"):
            u = _cached(weight, "wino", lambda: _wino_weights(L, w, Cin, Cout))
        # the epilogue leaves the following InstanceNorm's statistics (per-tile partial sums) where the form can
        nparts = 0
        if stats:
            nparts = (L.vqw_conv3x3_up2_fwd_stats_parts(Cin, Cout, N, h, wl) if form == "up2" else
                      L.vqw_conv3x3_wino_fwd_stats_parts(Cin, Cout, N, H, W) if form == "wino" else
                      L.vqw_conv3x3_wino_dil2_stats_parts(Cin, Cout, N, H, W) if form == "dil2" else
                      L.vqw_conv2d_fwd_stats_parts(x0.shape[1], c1, int(up0), N, H, W, Cout, ks, dilation))
        y = empty_nhwc(N, Cout, H, W, x0)
        part = torch.empty(N * nparts * Cout * 2, dtype=torch.float32, device=x0.device) if nparts > 0 else None
        if form == "up2" and part is not None:
            L.vqw_conv3x3_up2_fwd_stats(x0, up_ws, bias, y, part, N, h, wl, Cin, Cout)
        elif form == "up2":
            L.vqw_conv3x3_up2_fwd(x0, up_ws, bias, y, N, h, wl, Cin, Cout, int(relu))
        elif form == "wino" and part is not None:
            L.vqw_conv3x3_wino_fwd_stats(x0, u, bias, y, part, N, H, W, Cin, Cout)
        elif form == "wino":
            L.vqw_conv3x3_wino_fwd(x0, u, bias, y, N, H, W, Cin, Cout, int(relu))
        elif form == "dil2":
            L.vqw_conv3x3_wino_dil2_fwd(x0, u, bias, y, part, 0, N, H, W, Cin, Cout, int(relu))
        elif part is not None:
            L.vqw_conv2d_fwd_stats(x0, x0.shape[1], int(up0), x1, c1, w, bias, y, part, N, H, W, Cout, ks, dilation)
        else:
            L.vqw_conv2d_fwd(x0, x0.shape[1], int(up0), x1, c1, w, bias, y, N, H, W, Cout, ks, dilation, int(relu))
        ctx.up_ws = up_ws
        ctx.group = grad_group
        ctx.save_for_backward(x0, x1, w, y if relu else None)
        ctx.cfg = (dilation, up0, ks, N, H, W, Cout, bias is not None)
        # leaf parameters get their gradient written out-of-band on the side stream (see _deferred_wgrad)
        ctx.params = (weight, bias)
        ctx.defer = _out_of_band(ctx.needs_input_grad[2], ctx.params, w is weight)
        if want_stats:
            if part is not None:
                ctx.mark_non_differentiable(part)
            # (without this autograd hands backward a zero-filled "gradient" of the statistics partials: one fill launch per
            # convolution and step, 108 of them)
            ctx.set_materialize_grads(False)
            return y, part
        return y

    @staticmethod
    def backward(ctx, gy, *_):
        if gy is None:             # y itself was not used (only possible with gradient materialisation off)
            return (None,) * 11
        x0, x1, w, y_relu = ctx.saved_tensors
        dilation, up0, ks, N, H, W, Cout, has_bias = ctx.cfg
        need0, need1, needw, needb = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        defer = ctx.defer and (needw or (needb and has_bias))
        g0, g1, gw, gb, gy = conv2d_backward_impl(gy, x0, x1, w, y_relu, dilation, up0, has_bias, ctx.up_ws, need0, need1,
                                                  needw and not defer, needb and not defer, group=ctx.group, in_src=ctx.in_src)
        if defer:
            weight, bias = ctx.params
            _deferred_wgrad(weight, bias if (has_bias and bias.requires_grad) else None, x0, x1, gy, up0, ks, dilation,
                            N, H, W, Cout, collapsed=ctx.up_ws is not None)
        return g0, g1, gw, gb, None, None, None, None, None, None, None


class _GradNotes:
    """Notes that a consumer's input-gradient launch leaves for the producer's backward of the SAME backward pass, keyed by the
    gradient tensor it hands to autograd.  A note is honoured only when the tensor that reaches the producer is that very
    gradient, untouched: same address, same version counter (autograd's InputBuffer sums the gradients of a tensor with
    several consumers IN PLACE when it owns the first one - `old.add_(new)` keeps the address and bumps the version), same
    backward pass (addresses recur from step to step under the caching allocator).  Whatever is left at the end of a pass is
    dropped by an end-of-pass callback, and begin_step() drops it again (the engine skips callbacks behind one that raises)."""

    def __init__(self):
        self.notes = {}
        self._armed_for = None

    def put(self, grad, payload):
        tid = _pass_id()
        if tid >= 0 and self._armed_for != tid:      # (outside a backward pass nobody will take the note: begin_step() drops it)
            self._armed_for = tid
            torch.autograd.Variable._execution_engine.queue_callback(self.clear)
        self.notes[grad.data_ptr()] = (grad._version, tid, payload)

    def take(self, grad):
        ent = self.notes.pop(grad.data_ptr(), None)
        if ent is None or ent[0] != grad._version or ent[1] != _pass_id():
            return None
        return ent[2]

    def clear(self):
        self.notes.clear()
        self._armed_for = None

    def __len__(self):
        return len(self.notes)


# ----------------------------------------------------------------------------------------------
# two 3x3 layers of one input as ONE launch on concatenated weights:
#  - up-sampled: 32 couts each, one 64-cout launch (StyledResUpBlock's shortcut `conv` and `conv1`)
#  - plain: StyledResUpBlock's mlp_shared convolutions of its two StyledDenorms read the same style tensor (blocks.py:72-75 / 100-134)
# ----------------------------------------------------------------------------------------------
UP_PAIR = os.environ.get("VQW_UP_PAIR", "1") != "0"      # 0: the two layers run one by one (A/B timing)
up_pair_calls = 0
CONV_PAIR = os.environ.get("VQW_CONV_PAIR", "1") != "0"      # 0: the two layers run one by one (A/B timing)
conv_pair_calls = 0


class _ConvPair(torch.autograd.Function):
    """Two 3x3 layers a and b of one input x, computed by one launch on their concatenated weights.
    up=True: (y_a, part_a, y_b, part_b) = the forward of conv2d(x, w_a, b_a, up2x=True, want_stats=True) and of the same with
    (w_b, b_b), one launch of the nine-product kernel (a 32-cout layer alone falls back to the collapsed 4-tap form at a third
    of that kernel's rate).
    up=False: (y_a, y_b) = conv2d(x, w_a, b_a, relu=relu), conv2d(x, w_b, b_b, relu=relu) in Winograd form, one launch of the
    64-cout kernel with a two-tensor epilogue (vqw_conv3x3_wino_fwd_split): the input is read and transformed once, and two
    32-cout layers leave the 128-tile x 32-cout workgroup shape for the 64 x 64 one.
    The backward is the two layers' own: each input gradient through its layer's own weights (collapsed ones when up), the
    second added to the first in its kernel's epilogue when `group` is given, each weight gradient on the side lanes."""

    @staticmethod
    def forward(ctx, x, wa, ba, wb, bb, relu, group, up):
        global up_pair_calls, conv_pair_calls
        _dev(x, wa, ba, wb, bb)
        x = nhwc(x)
        Ca, Cin, ks, _ = wa.shape
        N, _, h, w = x.shape
        L = _L()
        deps = (wb,) + tuple(t for t in (ba, bb) if t is not None)
        if up:
            nparts = L.vqw_conv3x3_up2_fwd_pair_supported(Cin, Ca, N, h, w)
            if nparts <= 0 or tuple(wb.shape) != tuple(wa.shape) or ks != 3:
                raise RuntimeError("conv2d_up_pair: shape not served (query vqw_conv3x3_up2_fwd_pair_supported)")
            up_ws, bias_cat = _cached(wa, "up2pair", lambda: _concat_layers(wa, ba, wb, bb, lambda wc: _up2_weights(L, wc, Cin, 2 * Ca)),
                                      deps=deps)
            H, W = 2 * h, 2 * w
            ya = empty_nhwc(N, Ca, H, W, x)
            yb = empty_nhwc(N, Ca, H, W, x)
            pa = torch.empty(N * nparts * Ca * 2, dtype=torch.float32, device=x.device)
            pb = torch.empty(N * nparts * Ca * 2, dtype=torch.float32, device=x.device)
            L.vqw_conv3x3_up2_fwd_pair(x, up_ws, bias_cat, ya, yb, pa, pb, N, h, w, Cin, Ca)
            up_pair_calls += 1
            ctx.mark_non_differentiable(pa, pb)
            outs = (ya, pa, yb, pb)
        else:
            H, W = h, w
            if tuple(wb.shape) != tuple(wa.shape) or ks != 3 or (ba is None) != (bb is None) \
                    or not L.vqw_conv3x3_wino_split_supported(Cin, 2 * Ca, Ca, 0, N, H, W):
                raise RuntimeError("conv2d_pair: shape not served (query vqw_conv3x3_wino_split_supported)")
            u, bias_cat = _cached(wa, "pair_wino", lambda: _concat_layers(wa, ba, wb, bb, lambda wc: _wino_weights(L, wc, Cin, 2 * Ca)),
                                  deps=deps)
            ya = empty_nhwc(N, Ca, H, W, x)
            yb = empty_nhwc(N, Ca, H, W, x)
            L.vqw_conv3x3_wino_fwd_split(x, u, bias_cat, ya, yb, N, H, W, Cin, 2 * Ca, Ca, 0, int(relu))
            conv_pair_calls += 1
            outs = (ya, yb)
        wa_n, wb_n = nhwc(wa), nhwc(wb)
        ctx.save_for_backward(x, wa_n, wb_n, ya if relu else None, yb if relu else None)
        ctx.up = up
        ctx.group = group
        ctx.cfg = (N, H, W, Ca, Cin)
        ctx.params = ((wa, ba), (wb, bb))
        ctx.defer = [_out_of_band(ctx.needs_input_grad[1 + 2 * i], params, w_n is params[0])
                     for i, (params, w_n) in enumerate(zip(ctx.params, (wa_n, wb_n)))]
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        x, wa_n, wb_n, ya, yb = ctx.saved_tensors
        N, H, W, Cout, Cin = ctx.cfg
        up = ctx.up
        L = _L()
        out = [None] * 8
        gx_total = None
        # (the second layer's input gradient runs first, like the second of two separate nodes would)
        for i in (1, 0):
            gy = grads[2 * i] if up else grads[i]
            if gy is None:
                if ctx.group is not None:
                    raise RuntimeError("%s: both outputs must take part in the backward pass of a gradient group"
                                       % ("conv2d_up_pair" if up else "conv2d_pair"))
                continue
            wgt, bias = ctx.params[i]
            w_n = (wa_n, wb_n)[i]
            up_ws = _cached(wgt, "up2", lambda: _up2_weights(L, w_n, Cin, Cout)) if up else None
            need0 = ctx.needs_input_grad[0]
            needw, needb = ctx.needs_input_grad[1 + 2 * i], (bias is not None and ctx.needs_input_grad[2 + 2 * i])
            defer = ctx.defer[i] and (needw or needb)
            g0, _, gw, gbias, gy_n = conv2d_backward_impl(gy, x, None, w_n, (ya, yb)[i], 1, up, bias is not None, up_ws, need0, False,
                                                          needw and not defer, needb and not defer, group=ctx.group)
            if defer:
                _deferred_wgrad(wgt, bias if (bias is not None and bias.requires_grad) else None, x, None, gy_n, up, 3, 1,
                                N, H, W, Cout, collapsed=up)
            out[1 + 2 * i], out[2 + 2 * i] = gw, gbias
            if g0 is not None:
                gx_total = g0 if gx_total is None else gx_total.add_(g0)
        out[0] = gx_total
        return tuple(out)


def conv2d_up_pair_supported(x, weight_a, weight_b):
    """True when conv2d_up_pair serves these two layers (both 3x3, 32 couts, same shape, the nine-product kernel's geometry)."""
    if not (UP_PAIR and x.is_cuda and weight_a.shape == weight_b.shape and weight_a.shape[2] == 3 and not _in_custom_op):
        return False
    N, _, h, w = x.shape
    return _L().vqw_conv3x3_up2_fwd_pair_supported(weight_a.shape[1], weight_a.shape[0], N, h, w) > 0


def conv2d_up_pair(x, weight_a, bias_a, weight_b, bias_b, grad_group=None):
    """-> ((y_a, part_a), (y_b, part_b)): conv2d(x, w, b, up2x=True, want_stats=True) of two layers of one input, one launch."""
    ya, pa, yb, pb = _ConvPair.apply(x, weight_a, bias_a, weight_b, bias_b, False, grad_group if GRAD_GROUPS else None, True)
    return (ya, pa), (yb, pb)


def conv2d_pair_supported(x, weight_a, weight_b):
    """True when conv2d_pair serves these two layers here: both 3x3 of one shape, the Winograd forward admitted at this point of the
    graph (ops.winograd_forward() / evaluation), the 64-cout kernel's geometry."""
    if not (CONV_PAIR and x.is_cuda and weight_a.shape == weight_b.shape and weight_a.shape[2] == 3 and not _in_custom_op
            and _decide_wino_fwd()):
        return False
    N, _, H, W = x.shape
    Ca, Cin = weight_a.shape[0], weight_a.shape[1]
    L = _L()
    return bool(L.vqw_conv3x3_wino_supported(Cin, 2 * Ca, N, H, W) and L.vqw_conv3x3_wino_split_supported(Cin, 2 * Ca, Ca, 0, N, H, W))


def conv2d_pair(x, weight_a, bias_a, weight_b, bias_b, relu=False, grad_group=None):
    """-> (y_a, y_b): conv2d(x, w, b, relu=relu) of two 3x3 layers of one input, one launch."""
    return _ConvPair.apply(x, weight_a, bias_a, weight_b, bias_b, bool(relu), grad_group if GRAD_GROUPS else None, False)


# Gradients that arrive already multiplied by a fused ReLU's mask: payload = data_ptr of the ReLU output the gradient was masked
# with.  Written by a consumer whose input-gradient kernel applies the mask in its epilogue (vqw_conv3x3_wino_fwd_masked),
# taken by the producer's backward, which then skips its own mask pass.
_MASKED_GRADS = _GradNotes()
FUSE_RELU_MASK = os.environ.get("VQW_FUSE_RELU_MASK", "1") != "0"
# Norm-backward sums that a consumer convolution's input-gradient launch has left per region: payload = (partials, regions per
# image, data_ptr of the norm's raw input) - written by conv2d_backward_impl (vqw_conv3x3_wino_fwd_inbwd), taken by
# _InstanceNorm.backward, which then skips its reduction pass over the activation and the gradient.
_IN_BWD_PARTS = _GradNotes()
FUSE_IN_BWD = os.environ.get("VQW_FUSE_IN_BWD", "1") != "0"


# BatchNorm's num_batches_tracked counters (read by nobody on this path: momentum is a number, not None) are bumped by ONE
# multi-tensor launch at the end of a trainer's step instead of one launch per normalisation call; outside a trainer step
# (begin_step() ... join_streams()) every call bumps its counter at once.
_defer_counters = False
_pending_counters = []


def _bump_counter(t):
    if _defer_counters:
        _pending_counters.append(t)
    else:
        t.add_(1)


def flush_counters():
    global _pending_counters
    if _pending_counters:
        pend, _pending_counters = _pending_counters, []
        uniq, times = [], {}
        for t in pend:
            k = id(t)
            if k not in times:
                uniq.append(t)
            times[k] = times.get(k, 0) + 1
        by = {}
        for t in uniq:
            by.setdefault(times[id(t)], []).append(t)
        for n, ts in by.items():
            torch._foreach_add_(ts, n)


def begin_step():
    """Call before the forwards of a training step: drops fusion notes and a lane join that a failed backward pass left."""
    global _defer_counters
    flush_counters()               # (whatever an aborted step left)
    _defer_counters = True         # until join_streams()
    _MASKED_GRADS.clear()
    _IN_BWD_PARTS.clear()
    if _join_queued_for is not None:
        _join_side_stream()
    elif _fold_keep or _lib.load().vqw_fold_pending():      # a pass that never reached its lane join: its slabs are still alive
        sync_wgrad_lanes()
        _fold_flush()


in_bwd_fused_calls = 0         # InstanceNorm backward calls that took their sums from a convolution's epilogue (tests)
masked_dgrad_calls = 0         # input-gradient launches that applied a ReLU mask in their epilogue (tests)
group_acc_calls = 0            # Winograd input-gradient launches that added to a gradient group's buffer in their epilogue (tests)
split_dgrad_calls = 0          # two-source input-gradient launches whose epilogue wrote both sources' gradients (tests)
SPLIT_DGRAD = os.environ.get("VQW_SPLIT_DGRAD", "1") != "0"      # 0: concatenated gradient + two gather passes (A/B)


def conv2d_backward_impl(gy, x0, x1, w, y_relu, dilation, up0, has_bias, up_ws, need0, need1, needw, needb, group=None, in_src=None):
    """Input / weight / bias gradients of conv2d on the current stream -> (g0, g1, gw, gb, masked gy).  x0 / x1 / w are the
    NHWC tensors the forward saw, y_relu its output when the ReLU was fused (the incoming gradient is masked first),
    up_ws the collapsed-weight buffer when the forward took the low-resolution form."""
    global group_acc_calls, split_dgrad_calls, in_bwd_fused_calls
    L = _L()
    Cout, Cin, ks, _ = w.shape
    N = x0.shape[0]
    H, W = (x0.shape[2] * 2, x0.shape[3] * 2) if up0 else (x0.shape[2], x0.shape[3])
    masked_with = _MASKED_GRADS.take(gy) if y_relu is not None else None
    gy = nhwc(gy)
    if y_relu is not None:   # fused ReLU epilogue: mask the incoming gradient first
        if masked_with is not None and masked_with == y_relu.data_ptr():
            pass             # the consumer's input-gradient kernel has applied this very mask in its epilogue (_ConvCat.backward)
        else:
            gm = torch.empty_like(y_relu, memory_format=CL)
            L.vqw_relu_bwd(y_relu, gy, gm, gy.numel())
            gy = gm
    C0 = x0.shape[1]
    C1 = 0 if x1 is None else x1.shape[1]
    g0 = g1 = gw = gb = None

    # derived weights of the input-gradient convolution, kept on w while it is unchanged: U of its Winograd form (the Winograd
    # routes), the packed weights (the others)
    def wino_u():
        return _cached(w, "wino_dgrad", lambda: _wino_weights_dgrad(L, w, Cout, Cin))

    def packed():
        def _pack():
            buf = torch.empty(Cin * ks * ks * Cout, dtype=torch.float32, device=gy.device)
            L.vqw_pack_dgrad_weights(w, buf, Cout, Cin, ks)
            return buf
        return _cached(w, "dgrad", _pack)

    if need0 and up_ws is not None:
        if group is not None and group.buf is not None and L.vqw_conv3x3_up2_dgrad_acc_supported(Cin, Cout, N, H // 2, W // 2):
            # the other up-sampled convolution of this input has run: add to its gradient in this kernel's epilogue
            L.vqw_conv3x3_up2_dgrad_acc(gy, up_ws, group.buf, N, H // 2, W // 2, Cin, Cout)
            group_acc_calls += 1
            g0 = group.member_done(None)
        else:
            g0 = torch.empty_like(x0, memory_format=CL)
            L.vqw_conv3x3_up2_dgrad(gy, up_ws, g0, N, H // 2, W // 2, Cin, Cout)
            if group is not None:
                g0 = group.member_done(g0)
    elif need0 or (need1 and x1 is not None):
        # two sources [up2x(x0) | x1]: both gradients leave the input-gradient kernel's epilogue (x0's summed over each 2 x 2 tile
        # when x0 was up-sampled: a Winograd tile IS one low-resolution pixel) instead of two gather passes over the concatenated
        # gradient.  Cp: the input channels of that launch - the layer's own, or for a channel total that is not a multiple of the
        # kernel's cout tile (48 at the encoder's full-resolution level) the layer widened to 64 with zero weights, the padding
        # couts of the launch not stored
        Cp = None
        if SPLIT_DGRAD and x1 is not None and need0 and need1 and group is None and ks == 3 and dilation == 1:
            if L.vqw_conv3x3_wino_supported(Cout, Cin, N, H, W) and L.vqw_conv3x3_wino_split_supported(Cout, Cin, C0, int(up0), N, H, W):
                Cp = Cin
            elif Cin % 64 != 0 and C0 % 16 == 0 and C1 % 16 == 0:
                Cp = (Cin + 63) // 64 * 64
                if not (L.vqw_conv3x3_wino_supported(Cout, Cp, N, H, W)
                        and L.vqw_conv3x3_wino_split_padded_supported(Cout, Cp, C0, C1, int(up0), N, H, W)):
                    Cp = None
        if Cp is not None:
            if Cp == Cin:
                ut = wino_u()
            else:
                def _padded():
                    wp = torch.zeros((Cout, Cp, 3, 3), dtype=torch.float32, device=w.device).contiguous(memory_format=CL)
                    wp[:, :Cin].copy_(w.detach())
                    return _wino_weights_dgrad(L, wp, Cout, Cp)
                ut = _cached(w, "wino_dgrad_pad", _padded)
            g0 = torch.empty_like(x0, memory_format=CL)
            g1 = torch.empty_like(x1, memory_format=CL)
            if Cp == Cin:
                L.vqw_conv3x3_wino_fwd_split(gy, ut, None, g0, g1, N, H, W, Cout, Cin, C0, int(up0), 0)
            else:
                L.vqw_conv3x3_wino_fwd_split_padded(gy, ut, None, g0, g1, N, H, W, Cout, Cp, C0, C1, int(up0), 0)
            split_dgrad_calls += 1
        else:
            # a later member of a gradient group (single full-resolution source) adds into the shared buffer where a kernel can
            acc = group is not None and need0 and group.buf is not None
            g_full = None
            if acc and ks == 3 and dilation == 1 and L.vqw_conv3x3_wino_supported(Cout, Cin, N, H, W) \
                    and L.vqw_conv3x3_wino_masked_supported(Cout, Cin, N, H, W):
                # Winograd form, the shared buffer read and added in the kernel's epilogue
                L.vqw_conv3x3_wino_fwd_acc(gy, wino_u(), group.buf, N, H, W, Cout, Cin)
                group_acc_calls += 1
            elif acc and ks == 3 and dilation == 2 and L.vqw_conv3x3_wino_dil2_supported(Cout, Cin, N, H, W):
                # dilation 2: the Winograd kernel on the phase images, adding to the shared buffer in its epilogue
                L.vqw_conv3x3_wino_dil2_fwd(gy, wino_u(), None, group.buf, None, 1, N, H, W, Cout, Cin, 0)
            elif acc and L.vqw_conv2d_fwd_acc_supported(Cout, N, H, W, Cin, ks, dilation):
                # row-chain kernel (dilated 3x3) or the implicit-GEMM kernel (1x1): y += conv in the epilogue
                L.vqw_conv2d_fwd_acc(gy, Cout, packed(), group.buf, N, H, W, Cin, ks, dilation)
                if ks == 1:
                    group_acc_calls += 1
            else:
                g_full = empty_nhwc(N, Cin, H, W, gy)
                if in_src is not None and need0 and group is None and FUSE_IN_BWD \
                        and L.vqw_conv3x3_wino_fwd_inbwd_parts(Cout, Cin, N, H, W) > 0:
                    # x0 is the output of an InstanceNorm (+ReLU) and feeds this layer only: the norm's backward sums ride in this launch
                    nparts = L.vqw_conv3x3_wino_fwd_inbwd_parts(Cout, Cin, N, H, W)
                    ut = wino_u()
                    bpart = torch.empty(N * nparts * Cin * 2, dtype=torch.float32, device=gy.device)
                    xraw, mr, nrelu = in_src
                    L.vqw_conv3x3_wino_fwd_inbwd(gy, ut, xraw, mr, int(nrelu), g_full, bpart, N, H, W, Cout, Cin)
                    _IN_BWD_PARTS.put(g_full, (bpart, nparts, xraw.data_ptr()))
                elif ks == 3 and dilation == 1 and L.vqw_conv3x3_wino_supported(Cout, Cin, N, H, W):
                    L.vqw_conv3x3_wino_fwd(gy, wino_u(), None, g_full, N, H, W, Cout, Cin, 0)
                elif ks == 3 and dilation == 2 and x1 is None and not up0 and L.vqw_conv3x3_wino_dil2_supported(Cout, Cin, N, H, W):
                    L.vqw_conv3x3_wino_dil2_fwd(gy, wino_u(), None, g_full, None, 0, N, H, W, Cout, Cin, 0)
                else:
                    L.vqw_conv2d_fwd(gy, Cout, 0, None, 0, packed(), None, g_full, N, H, W, Cin, ks, dilation, 0)
            if group is not None and need0:
                g0 = group.member_done(g_full)
            elif not up0 and x1 is None:
                g0 = g_full
            else:
                if need0:
                    g0 = torch.empty_like(x0, memory_format=CL)
                    L.vqw_input_grad_gather(g_full, Cin, 0, C0, int(up0), g0, 0, N, H, W)
                if need1 and x1 is not None:
                    g1 = torch.empty_like(x1, memory_format=CL)
                    L.vqw_input_grad_gather(g_full, Cin, C0, C1, 0, g1, 0, N, H, W)
    if needw or (needb and has_bias):
        gw = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=gy.device, memory_format=CL)
        gb = torch.empty(Cout, dtype=torch.float32, device=gy.device) if has_bias else None
        _run_wgrad(L, x0, x1, gy, gw, gb, up0, ks, dilation, N, H, W, Cout, False, up_ws is not None)
    return g0, g1, gw, gb, gy


class GradGroup:
    """Several convolutions of ONE input tensor whose input gradients are summed in place instead of by autograd
    (aspp.py:44-47: the pyramid's five branches).  Every member's backward adds its input gradient to one shared buffer
    and returns None for the input, except the last one to run, which returns the buffer: autograd sees a single gradient
    and launches no add kernels (three passes over the tensor each).  All members must take part in every backward pass
    over the graph (their outputs are all used) and run on one stream.  The group re-arms itself when its last member has
    run, so a second pass over a retained graph works; a pass in which only SOME members ran (torch.autograd.grad over part
    of the branch outputs) cannot hand the input its gradient and raises at the end of that pass instead of dropping it."""

    def __init__(self, members):
        self.members = self.remaining = int(members)
        self.buf = None
        self._watching = False

    def opt_out(self):
        """A member whose input gradient goes through autograd after all (no accumulating route for its form)."""
        self.members -= 1
        self.remaining -= 1

    def member_done(self, g_full):
        """Called by a member's backward with its input gradient (None: already added to the buffer by the kernel).
        Returns what the member hands to autograd: the summed buffer from the last member to run, None from the others."""
        if not self._watching:             # first member of this pass: check completeness when the pass ends
            self._watching = True
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_pass)
        if self.buf is None:
            self.buf = g_full                     # first member to run: its gradient is the buffer
        elif g_full is not None:
            self.buf.add_(g_full)                 # no accumulating kernel for this member's shape
        self.remaining -= 1
        if self.remaining < 0:
            raise RuntimeError("GradGroup: more backward calls than members")
        if self.remaining > 0:
            return None
        out, self.buf, self.remaining = self.buf, None, self.members          # complete: re-armed for another pass
        return out

    def _end_of_pass(self):
        self._watching = False
        if self.buf is not None or self.remaining != self.members:
            ran = self.members - self.remaining
            self.buf, self.remaining = None, self.members
            # the engine skips every callback queued behind one that raises: do the lane join and drop the fusion notes here
            _join_side_stream()
            _MASKED_GRADS.clear()
            _IN_BWD_PARTS.clear()
            raise RuntimeError("GradGroup: only %d of %d members took part in this backward pass - their shared input "
                               "gradient was not delivered (partial backward over grouped branches: set VQW_GRAD_GROUPS=0)"
                               % (ran, self.members))


GRAD_GROUPS = os.environ.get("VQW_GRAD_GROUPS", "1") != "0"      # 0: autograd sums the branch gradients (A/B timing)


def conv2d(x, weight, bias=None, dilation=1, up2x=False, skip=None, relu=False, want_stats=False, grad_group=None, norm_input=False):
    """'same' conv (k in {1,3}, stride 1) of the virtual input [up2x(x) | skip] (channel concat);
    relu=True fuses nn.ReLU into the epilogue.  want_stats=True returns (y, part): `part` (or None when the shape is not
    served) holds the statistics of y for the InstanceNorm that follows: instance_norm(y, ..., part=part)."""
    wino = _decide_wino_fwd()
    group = grad_group if (GRAD_GROUPS and skip is None and not up2x) else None
    if grad_group is not None and group is None and GRAD_GROUPS and up2x and skip is None and weight.shape[2] == 3 and dilation == 1:
        # an up-sampled single source in its collapsed form (the branch _Conv2d.forward takes for these shapes)
        Cout_, Cin_ = weight.shape[0], weight.shape[1]
        if _L().vqw_conv3x3_up2_supported(Cin_, Cout_, x.shape[0], x.shape[2], x.shape[3]):
            group = grad_group
    if grad_group is not None and group is None:
        grad_group.opt_out()               # this member's gradient goes through autograd: the others must not wait for it
    # norm_input=True: x is the output of instance_norm(...) and feeds this layer ONLY - its input-gradient launch then also
    # leaves that norm's backward sums (a gradient that autograd had to sum with another consumer's would miss them)
    in_src = getattr(x, "_vqw_in_src", None) if (norm_input and FUSE_IN_BWD) else None
    if want_stats:
        return _Conv2d.apply(x, skip, weight, bias, int(dilation), bool(up2x), bool(relu), True, wino, group, in_src)
    return _Conv2d.apply(x, skip, weight, bias, int(dilation), bool(up2x), bool(relu), False, wino, group, in_src)


# ----------------------------------------------------------------------------------------------
# two 3x3 convs of the same input as ONE conv with concatenated output channels (StyledDenorm's mlp_gamma | mlp_beta):
# one pass over the input and twice the N-width per tile in forward, one K=2C dgrad whose accumulator sums the two
# input gradients (no add pass), one wgrad.  The parameters stay the two reference tensors; their .grad are the two
# halves of one buffer.
# ----------------------------------------------------------------------------------------------
def _cat_weights(wa, ba, wb, bb):
    return _cached(wa, "cat", lambda: _concat_layers(wa, ba, wb, bb), deps=(wb, ba, bb))


def _grad_halves_adjacent(pa, pb, ga, gb_):
    """True when pa.grad / pb.grad are the two halves of the buffer this module allocated."""
    buf = pa.__dict__.get("_vqw_gcat")
    return (buf is not None and ga is not None and gb_ is not None and ga.data_ptr() == buf.data_ptr()
            and gb_.data_ptr() == buf.data_ptr() + ga.numel() * 4 and ga.numel() + gb_.numel() == buf.numel())


def _deferred_wgrad_cat(wa, ba, wb, bb, x0, gy, ks, N, H, W):
    L = _L()
    Ca, Cin = wa.shape[0], wa.shape[1]
    Ct = Ca + wb.shape[0]
    with _side_lane(wa, (x0, gy), (wa, ba, wb, bb)):
        fresh = wa.grad is None and wb.grad is None and ba.grad is None and bb.grad is None
        if fresh:
            gw = torch.empty((Ct, Cin, ks, ks), dtype=torch.float32, device=gy.device, memory_format=CL)
            gb_ = torch.empty(Ct, dtype=torch.float32, device=gy.device)
            wa.grad, wb.grad, ba.grad, bb.grad = gw[:Ca], gw[Ca:], gb_[:Ca], gb_[Ca:]
            wa._vqw_gcat, ba._vqw_gcat = gw, gb_
            _run_wgrad(L, x0, None, gy, gw, gb_, False, ks, 1, N, H, W, Ct, False, False, defer_fold=True)
        elif _grad_halves_adjacent(wa, wb, wa.grad, wb.grad) and _grad_halves_adjacent(ba, bb, ba.grad, bb.grad):
            _run_wgrad(L, x0, None, gy, wa._vqw_gcat, ba._vqw_gcat, False, ks, 1, N, H, W, Ct, True, False, defer_fold=True)
        else:    # gradients someone else allocated: compute once, then accumulate the halves
            gw = torch.empty((Ct, Cin, ks, ks), dtype=torch.float32, device=gy.device, memory_format=CL)
            gb_ = torch.empty(Ct, dtype=torch.float32, device=gy.device)
            _run_wgrad(L, x0, None, gy, gw, gb_, False, ks, 1, N, H, W, Ct, False, False)
            for p, g in ((wa, gw[:Ca]), (wb, gw[Ca:]), (ba, gb_[:Ca]), (bb, gb_[Ca:])):
                if p.grad is None:
                    p.grad = g
                else:
                    p.grad.add_(g)


class _ConvCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wa, ba, wb, bb, wino_fwd=False, relu_in=False):
        _dev(x, wa, ba, wb, bb)
        ctx.relu_in = bool(relu_in)       # x is the output of a fused ReLU and has no other consumer
        x = nhwc(x)
        Ca, Cin, ks, _ = wa.shape
        Cb = wb.shape[0]
        N, _, H, W = x.shape
        if x.shape[1] != Cin or tuple(wb.shape[1:]) != (Cin, ks, ks):
            raise RuntimeError("conv2d_cat: shapes %s / %s / %s do not match" % (tuple(x.shape), tuple(wa.shape), tuple(wb.shape)))
        w, b = _cat_weights(wa, ba, wb, bb)
        if wino_fwd and ks == 3 and _L().vqw_conv3x3_wino_supported(Cin, Ca + Cb, N, H, W):
            L = _L()
            u = _cached(wa, "cat_wino", lambda: _wino_weights(L, w, Cin, Ca + Cb), deps=(wb,))
            y = empty_nhwc(N, Ca + Cb, H, W, x)
            L.vqw_conv3x3_wino_fwd(x, u, b, y, N, H, W, Cin, Ca + Cb, 0)
        else:
            y = empty_nhwc(N, Ca + Cb, H, W, x)
            _L().vqw_conv2d_fwd(x, Cin, 0, None, 0, w, b, y, N, H, W, Ca + Cb, ks, 1, 0)
        ctx.save_for_backward(x, w)
        ctx.cfg = (ks, N, H, W, Ca, Cb)
        ctx.params = (wa, ba, wb, bb)
        ctx.defer = _out_of_band(all(ctx.needs_input_grad[1:5]), ctx.params, nhwc(wa) is wa and nhwc(wb) is wb)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        ks, N, H, W, Ca, Cb = ctx.cfg
        wa, ba, wb, bb = ctx.params
        Ct, Cin = Ca + Cb, x.shape[1]
        L = _L()
        gy = nhwc(gy)
        gx = gwa = gba = gwb = gbb = None
        if ctx.needs_input_grad[0]:
            def _pack():
                buf = torch.empty(Cin * ks * ks * Ct, dtype=torch.float32, device=gy.device)
                L.vqw_pack_dgrad_weights(w, buf, Ct, Cin, ks)
                return buf
            gx = empty_nhwc(N, Cin, H, W, gy)
            if ks == 3 and L.vqw_conv3x3_wino_supported(Ct, Cin, N, H, W):
                ut = _cached(wa, "cat_wino_dgrad", lambda: _wino_weights_dgrad(L, w, Ct, Cin), deps=(wb,))
                if ctx.relu_in and FUSE_RELU_MASK and L.vqw_conv3x3_wino_masked_supported(Ct, Cin, N, H, W):
                    # the gradient in FRONT of the producer's ReLU: its mask (x > 0) applied in this kernel's epilogue
                    L.vqw_conv3x3_wino_fwd_masked(gy, ut, x, gx, N, H, W, Ct, Cin)
                    _MASKED_GRADS.put(gx, x.data_ptr())
                    global masked_dgrad_calls
                    masked_dgrad_calls += 1
                else:
                    L.vqw_conv3x3_wino_fwd(gy, ut, None, gx, N, H, W, Ct, Cin, 0)
            else:
                wt = _cached(wa, "cat_dgrad", _pack, deps=(wb,))
                L.vqw_conv2d_fwd(gy, Ct, 0, None, 0, wt, None, gx, N, H, W, Cin, ks, 1, 0)
        if ctx.defer:
            _deferred_wgrad_cat(wa, ba, wb, bb, x, gy, ks, N, H, W)
        elif any(ctx.needs_input_grad[1:5]):
            gw = torch.empty((Ct, Cin, ks, ks), dtype=torch.float32, device=gy.device, memory_format=CL)
            gb_ = torch.empty(Ct, dtype=torch.float32, device=gy.device)
            _run_wgrad(L, x, None, gy, gw, gb_, False, ks, 1, N, H, W, Ct, False, False)
            gwa, gwb, gba, gbb = gw[:Ca], gw[Ca:], gb_[:Ca], gb_[Ca:]
        return gx, gwa, gba, gwb, gbb, None, None


def conv2d_cat(x, weight_a, bias_a, weight_b, bias_b, relu_input=False):
    """[conv(x, weight_a, bias_a) | conv(x, weight_b, bias_b)] along channels (3x3 / 1x1, stride 1, 'same').
    relu_input=True: x is the output of conv2d(..., relu=True) and feeds nothing else - the input gradient then leaves this
    node already masked by that ReLU (one kernel epilogue instead of a separate pass over the gradient)."""
    return _ConvCat.apply(x, weight_a, bias_a, weight_b, bias_b, _decide_wino_fwd(), bool(relu_input))


# ----------------------------------------------------------------------------------------------
# InstanceNorm (+ReLU)
# ----------------------------------------------------------------------------------------------
class _InstanceNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, relu, eps, part=None):
        _dev(x)
        x = nhwc(x)
        y = torch.empty_like(x, memory_format=CL)
        mr = _inorm_fwd(x, y, x.shape[1], 0, part, eps, relu)
        ctx.save_for_backward(x, mr)
        ctx.relu = relu
        ctx.mark_non_differentiable(mr)
        ctx.set_materialize_grads(False)
        return y, mr               # mr = (mean, rstd) per (image, channel): for a consumer that fuses this norm's backward sums

    @staticmethod
    def backward(ctx, gy, _gmr=None):
        if gy is None:
            return None, None, None, None
        x, mr = ctx.saved_tensors
        N, C, H, W = x.shape
        L = _L()
        ent = _IN_BWD_PARTS.take(gy)
        gy = nhwc(gy)
        if ent is not None and ent[2] == x.data_ptr():
            # the only consumer's input-gradient launch has left (sum gm, sum gm * xhat) per region: no reduction pass
            global in_bwd_fused_calls
            in_bwd_fused_calls += 1
            bpart, nparts, _ = ent
            gx = torch.empty_like(x, memory_format=CL)
            means = torch.empty(N * C * 2, dtype=torch.float32, device=x.device)
            L.vqw_inorm_bwd_parts(x, mr, gy, bpart, nparts, means, gx, N, H * W, C, int(ctx.relu))
            return gx, None, None, None
        return _inorm_bwd(x, mr, gy, ctx.relu), None, None, None


def instance_norm(x, relu=False, eps=1e-5, part=None):
    """part: statistics partials from conv2d(..., want_stats=True) of the SAME tensor (skips the reduction pass).
    The result carries `_vqw_in_src` = (raw input, relu): a convolution that is this tensor's ONLY consumer can be told so
    (conv2d(..., norm_input=True)) and then leaves the norm's backward sums in its input-gradient epilogue."""
    y, mr = _InstanceNorm.apply(x, bool(relu), float(eps), part)
    if FUSE_IN_BWD and torch.is_grad_enabled() and y.requires_grad:
        y._vqw_in_src = (nhwc(x), mr, bool(relu))
    return y


class _InstanceNormCat(torch.autograd.Function):
    """InstanceNorm(+ReLU) of several tensors written straight into the channel slices of ONE output
    (the torch.cat of aspp.py:47 is never materialised as a separate pass)."""

    @staticmethod
    def forward(ctx, relu, eps, parts, *xs):
        _dev(*xs)
        xs = [nhwc(x) for x in xs]
        N, _, H, W = xs[0].shape
        Ct = sum(x.shape[1] for x in xs)
        y = empty_nhwc(N, Ct, H, W, xs[0])
        mrs, off = [], 0
        for x in xs:
            if x.shape[0] != N or x.shape[2] != H or x.shape[3] != W:
                raise RuntimeError("instance_norm_cat: shape mismatch")
            part = parts[len(mrs)] if parts is not None else None
            mrs.append(_inorm_fwd(x, y, Ct, off, part, eps, relu))
            off += x.shape[1]
        ctx.save_for_backward(*xs, *mrs)
        ctx.relu, ctx.n = relu, len(xs)
        return y

    @staticmethod
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        xs, mrs = saved[:ctx.n], saved[ctx.n:]
        gy = nhwc(gy)
        Ct = gy.shape[1]
        outs, off = [], 0
        for x, mr in zip(xs, mrs):
            outs.append(_inorm_bwd(x, mr, gy, ctx.relu, Ct, off))
            off += x.shape[1]
        return (None, None, None, *outs)


def instance_norm_cat(xs, relu=True, eps=1e-5, parts=None):
    """parts: per input, the statistics partials of conv2d(..., want_stats=True) or None."""
    return _InstanceNormCat.apply(bool(relu), float(eps), tuple(parts) if parts is not None else None, *xs)


# ----------------------------------------------------------------------------------------------
# StyledDenorm core: BatchNorm2d(affine=False)(x) * (1 + gamma) + beta (+ReLU)
# ----------------------------------------------------------------------------------------------
# VQW_DP_FORCE=1 (or force_collectives(True)): issue every data-parallel collective - SyncBN statistics, VQ statistics, the
# gradient buckets of trainers.GradientAllReducer - also in a process group of ONE rank.  A one-GPU box can then run the
# real RCCL code path (ProcessGroupNCCL's stream / event ordering against the two view streams and the weight-gradient
# lanes); with one rank every all-reduce is the identity, so the step must equal the non-distributed step bit for bit
# (tests/test_gpu_dp.py::test_rccl_world_size_one_equals_plain_step).
FORCE_COLLECTIVES = os.environ.get("VQW_DP_FORCE", "0") == "1"
collective_calls = 0           # small collectives issued from this module since import (tools/dp_probe prints it per step)


def force_collectives(on=True):
    global FORCE_COLLECTIVES
    old, FORCE_COLLECTIVES = FORCE_COLLECTIVES, bool(on)
    return old


def _dist_on():
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or FORCE_COLLECTIVES)


def _all_reduce(t):
    global collective_calls
    collective_calls += 1
    dist.all_reduce(t)


class _Spade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, sync, nbt, res=None, part=None,
                res_norm=None):
        """res_norm = (statistics partials of res or None, relu, eps): `res` is the RAW input of an InstanceNorm(+ReLU) whose output is
        the residual; it is normalised inside the modulation kernel (vqw_spade_fwd_res_norm) and never materialised."""
        _dev(x, gamma, beta, res)
        x, gamma = nhwc(x), nhwc(gamma)
        N, C, H, W = x.shape
        # beta=None: `gamma` holds [gamma | beta] as 2C channels (conv2d_cat)
        fused = beta is None
        if fused:
            if gamma.shape[1] != 2 * C:
                raise RuntimeError("spade_norm: fused gamma|beta map needs %d channels, got %d" % (2 * C, gamma.shape[1]))
        else:
            beta = nhwc(beta)
        gbs = 2 * C if fused else C
        gptr = gamma
        bptr = gamma.narrow(1, C, C) if fused else beta      # fused: beta = channels C..2C of the same NHWC map
        L = _L()
        mr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        count = float(N * H * W)
        if training:
            sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
            fused_finalize = part is not None and not (sync and _dist_on())
            if fused_finalize:      # no collective between the sums and the statistics: one launch for both (below)
                pass
            elif part is not None:    # per-tile sums left by the producing convolution's epilogue
                rows = part.numel() // (2 * C)
                L.vqw_bn_stats_from_parts(part, sums, rows, C, count / rows)
            else:
                ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
                L.vqw_bn_partial_stats(x, sums, ws, ws.numel(), N, H * W, C)
            if sync and _dist_on():
                # SyncBatchNorm semantics (run_vqwnet.py:121): global-batch statistics, one small all-reduce.
                # Every rank holds the same per-rank batch (weak scaling), so the count needs no exchange.
                _all_reduce(sums)
                count *= dist.get_world_size()
            cur = _order_begin(running_mean)
            if fused_finalize:
                rows = part.numel() // (2 * C)
                L.vqw_bn_finalize_parts(part, rows, count / rows, sums, count, mr,
                                        running_mean, running_var, momentum, eps, C)
            else:
                L.vqw_bn_finalize(sums, count, mr, running_mean, running_var, momentum, eps, C)
            if nbt is not None:
                _bump_counter(nbt)
            _order_end(running_mean, cur)
        else:
            L.vqw_bn_eval_stats(running_mean, running_var, mr, eps, C)
        y = torch.empty_like(x, memory_format=CL)
        rmr = None
        if res is not None:         # y = act(...) + res: the block's `shortcut + main` inside this kernel
            res = nhwc(res)
            if res.shape != x.shape:
                raise RuntimeError("spade_norm: residual shape %s does not match %s" % (tuple(res.shape), tuple(x.shape)))
        if res is not None and res_norm is not None:
            rpart, rrelu, reps = res_norm
            rmr = _mean_rstd(res, rpart, reps)
            L.vqw_spade_fwd_res_norm(x, mr, gptr, bptr, gbs, res, rmr, int(rrelu), y, N, H * W, C, int(relu))
            ctx.res_relu = bool(rrelu)
        elif res is not None:
            L.vqw_spade_fwd_res(x, mr, gptr, bptr, gbs, res, y, N * H * W, C, int(relu))
        else:
            L.vqw_spade_fwd(x, mr, gptr, bptr, gbs, y, N * H * W, C, int(relu))
        ctx.save_for_backward(x, gamma, beta, mr, res if rmr is not None else None, rmr)
        ctx.cfg = (training, relu, count, sync, fused)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mr, res_raw, rmr = ctx.saved_tensors
        training, relu, count, sync, fused = ctx.cfg
        N, C, H, W = x.shape
        L = _L()
        gy = nhwc(gy)
        if fused:
            dgamma, dbeta, gbs = torch.empty_like(gamma, memory_format=CL), None, 2 * C
            gptr, dgptr = gamma, dgamma
            bptr, dbptr = gamma.narrow(1, C, C), dgamma.narrow(1, C, C)
        else:
            dgamma = torch.empty_like(x, memory_format=CL)
            dbeta = torch.empty_like(x, memory_format=CL)
            gbs, gptr, bptr, dgptr, dbptr = C, gamma, beta, dgamma, dbeta
        gx = torch.empty_like(x, memory_format=CL)
        sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
        ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
        L.vqw_spade_bwd_reduce(x, mr, gptr, bptr, gy, dgptr, dbptr, gbs, sums, ws, ws.numel(), N, H * W, C, int(relu))
        if training and sync and _dist_on():
            _all_reduce(sums)
        L.vqw_spade_bwd_apply(x, mr, gptr, bptr, gbs, gy, sums, count, gx, N * H * W, C, int(relu), int(training))
        gres = gy if ctx.has_res else None
        if rmr is not None and ctx.needs_input_grad[11]:
            # the residual was normalised in the forward kernel: its gradient goes back through that InstanceNorm(+ReLU) here
            gres = _inorm_bwd(res_raw, rmr, gy, ctx.res_relu)
        return gx, dgamma, dbeta, None, None, None, None, None, None, None, None, gres, None, None


RES_NORM_FUSED = os.environ.get("VQW_RES_NORM_FUSED", "1") != "0"      # 0: the shortcut's norm writes its tensor first (A/B)


def spade_norm(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, relu=False, sync=True,
               num_batches_tracked=None, residual=None, part=None, residual_norm=None):
    """residual: added AFTER the activation (y = act(spade(x)) + residual); needs C % 4 == 0.
    part: statistics partials of x from conv2d(..., want_stats=True) (training mode skips its reduction pass).
    residual_norm = (partials or None, relu, eps): `residual` is the RAW input of an InstanceNorm(+ReLU) - the block's shortcut
    branch - and is normalised inside the modulation kernel where the shape allows, by a separate pass otherwise."""
    if residual is not None and residual_norm is not None:
        N, C, H, W = x.shape
        if not (RES_NORM_FUSED and x.is_cuda and not (C & 3) and not (gamma.shape[1] & 3) and tuple(residual.shape) == tuple(x.shape)
                and _L().vqw_spade_fwd_res_norm_supported(H * W, C)):
            rpart, rrelu, reps = residual_norm
            residual = instance_norm(residual, relu=rrelu, eps=reps, part=rpart)
            residual_norm = None
    if residual_norm is not None:
        return _Spade.apply(x, gamma, beta, running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu),
                            bool(sync), num_batches_tracked, residual, part if training else None,
                            (residual_norm[0], bool(residual_norm[1]), float(residual_norm[2])))
    if residual is not None and (x.shape[1] & 3 or gamma.shape[1] & 3):
        return add(spade_norm(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, sync,
                              num_batches_tracked, part=part), residual)
    return _Spade.apply(x, gamma, beta, running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu),
                        bool(sync), num_batches_tracked, residual, part if training else None)


# ----------------------------------------------------------------------------------------------
# element-wise / pooling
# ----------------------------------------------------------------------------------------------
class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, relu, a_group=None):
        _dev(a, b)
        a, b = nhwc(a), nhwc(b)
        if a.shape != b.shape:
            raise RuntimeError("add: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty_like(a, memory_format=CL)
        _L().vqw_add(a, b, y, a.numel(), int(relu))
        ctx.relu = relu
        ctx.a_group = a_group
        if relu:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.relu:
            (y,) = ctx.saved_tensors
            gy = nhwc(gy)
            gx = torch.empty_like(y, memory_format=CL)
            _L().vqw_relu_bwd(y, gy, gx, y.numel())
            gy = gx
        if ctx.a_group is not None:
            # `a` has further consumers that form a gradient group (their backward runs AFTER everything upstream of `b`, which
            # reads this gradient, has run): this gradient is the group's member - as the first to arrive it becomes the buffer
            # the others add to in their kernels' epilogues; the last member hands the sum to autograd
            return ctx.a_group.member_done(nhwc(gy)), gy, None, None
        return gy, gy, None, None


class _AddNorm(torch.autograd.Function):
    """y = a + InstanceNorm(+ReLU)(x) with x the RAW convolution output and `part` its statistics partials (or None): the norm is
    applied inside the add's kernel (vqw_inorm_add_fwd), its output never written.  Backward: the gradient of `a` is gy (handed to
    `a_group` like _Add does), the gradient of x is the norm's backward of gy."""

    @staticmethod
    def forward(ctx, a, x, part, relu, eps, a_group):
        _dev(a, x)
        a, x = nhwc(a), nhwc(x)
        if a.shape != x.shape:
            raise RuntimeError("add_norm: shape mismatch %s vs %s" % (tuple(a.shape), tuple(x.shape)))
        N, C, H, W = x.shape
        L = _L()
        mr = _mean_rstd(x, part, eps)
        y = torch.empty_like(x, memory_format=CL)
        L.vqw_inorm_add_fwd(x, mr, a, y, N, H * W, C, int(relu))
        ctx.save_for_backward(x, mr)
        ctx.relu, ctx.a_group = bool(relu), a_group
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mr = ctx.saved_tensors
        gy = nhwc(gy)
        gx = _inorm_bwd(x, mr, gy, ctx.relu) if ctx.needs_input_grad[1] else None
        ga = gy
        if ctx.a_group is not None:
            ga = ctx.a_group.member_done(gy)
        return ga, gx, None, None, None, None


def add_norm_supported(a, x):
    return bool(x.is_cuda and x.dim() == 4 and tuple(a.shape) == tuple(x.shape) and _L().vqw_inorm_add_supported(x.shape[1]))


def add_norm(a, x, part=None, relu=False, eps=1e-5, a_group=None):
    """a + instance_norm(x, relu, eps, part) in one kernel (see _AddNorm); query add_norm_supported first."""
    return _AddNorm.apply(a, x, part, bool(relu), float(eps), a_group)


def add(a, b, relu=False, a_group=None):
    """a + b (+ReLU).  a_group: an ops.GradGroup that the OTHER consumers of `a` belong to, sized for them plus this op; `b`
    must be computed from `a` through those consumers (x + f(x)), so that their backward runs after b's whole chain."""
    return _Add.apply(a, b, bool(relu), a_group)


# ----------------------------------------------------------------------------------------------
# VQGAN decoder blocks (networks/vqgan.py): GroupNorm(32)(+swish) and single-head self-attention
# ----------------------------------------------------------------------------------------------
class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, swish):
        _dev(x, weight, bias)
        x = nhwc(x)
        weight, bias = _flat(weight), _flat(bias)
        N, C, H, W = x.shape
        if C % 32 != 0 or weight.numel() != C or bias.numel() != C:
            raise RuntimeError("group_norm: num_channels (%d) must be divisible by num_groups (32), weight / bias of that size" % C)
        L = _L()
        y = torch.empty_like(x, memory_format=CL)
        mean = torch.empty(N, 32, dtype=torch.float32, device=x.device)
        rstd = torch.empty(N, 32, dtype=torch.float32, device=x.device)
        ws = _ws(L.vqw_groupnorm_ws_bytes(N, H * W, C), x)
        L.vqw_groupnorm_fwd(x, weight, bias, y, mean, rstd, ws, ws.numel(), N, H * W, C, eps, int(swish))
        ctx.save_for_backward(x, weight, bias, mean, rstd)      # not the pre-activation: the backward recomputes it
        ctx.swish = swish
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        N, C, H, W = x.shape
        L = _L()
        gy = nhwc(gy)
        gx = torch.empty_like(x, memory_format=CL)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _ws(L.vqw_groupnorm_ws_bytes(N, H * W, C), x)
        L.vqw_groupnorm_bwd(x, weight, bias, mean, rstd, gy, gx, dgamma, dbeta, ws, ws.numel(), N, H * W, C, int(ctx.swish))
        return gx, dgamma, dbeta, None, None


def group_norm(x, weight, bias, eps=1e-6, swish=False):
    """nn.GroupNorm(32, C, eps, affine=True)(x), with swish=True followed by y * sigmoid(y), as one pass."""
    return _GroupNorm.apply(x, weight, bias, float(eps), bool(swish))


class _Swish(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = nhwc(x) if x.dim() == 4 else _flat(x)
        y = torch.empty_like(x)
        _L().vqw_swish_fwd(x, y, x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = nhwc(gy) if x.dim() == 4 else _flat(gy)
        gx = torch.empty_like(x)
        _L().vqw_swish_bwd(x, gy, gx, x.numel())
        return gx


def swish(x):
    """x * sigmoid(x) on its own; behind a GroupNorm use group_norm(..., swish=True) instead."""
    return _Swish.apply(x)


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        _dev(q, k, v)
        if not (q.shape == k.shape == v.shape):
            raise RuntimeError("self_attention: q, k, v must have one shape (got %s, %s, %s)" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        q, k, v = nhwc(q), nhwc(k), nhwc(v)
        B, C, H, W = q.shape
        o = torch.empty_like(q, memory_format=CL)
        lse = torch.empty(B, H * W, dtype=torch.float32, device=q.device)
        _L().vqw_attention_fwd(q, k, v, o, lse, B, H * W, C, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        B, C, H, W = q.shape
        go = nhwc(go)
        gq, gk, gv = (torch.empty_like(q, memory_format=CL) for _ in range(3))
        d = torch.empty_like(lse)
        _L().vqw_attention_bwd(q, k, v, o, lse, go, d, gq, gk, gv, B, H * W, C, ctx.scale)
        return gq, gk, gv, None


def self_attention(q, k, v, scale):
    """softmax(scale * q^T k) applied to v over the H*W positions of three (B, C, H, W) maps of one shape (the reference's
    AttnBlock, vqgan.py:163-176); returns a map of that shape.  The (HW x HW) score matrix is never materialised."""
    return _SelfAttention.apply(q, k, v, float(scale))


def self_attention_lse(q, k, v, scale):
    """(output, row log-sum-exp [B, H*W]) of self_attention without a tape: for tests and measurement."""
    _dev(q, k, v)
    q, k, v = nhwc(q), nhwc(k), nhwc(v)
    B, C, H, W = q.shape
    o = torch.empty_like(q, memory_format=CL)
    lse = torch.empty(B, H * W, dtype=torch.float32, device=q.device)
    _L().vqw_attention_fwd(q, k, v, o, lse, B, H * W, C, float(scale))
    return o, lse


# ----------------------------------------------------------------------------------------------
# minGPT blocks (networks/mingpt.py): LayerNorm, exact GELU, nn.Linear, multi-head causal attention on (B, T, C) tensors
# ----------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _dev(x, weight, bias)
        x, weight, bias = _flat(x), _flat(weight), _flat(bias)
        C = x.shape[-1] if x.dim() >= 1 else 0
        if weight.numel() != C or bias.numel() != C:
            raise RuntimeError("layer_norm: weight / bias of %d / %d elements for a trailing dimension of %d" % (weight.numel(), bias.numel(), C))
        rows = x.numel() // max(C, 1)
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _L().vqw_layernorm_fwd(x, weight, bias, y, mean, rstd, rows, C, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, rstd = ctx.saved_tensors
        C, rows = x.shape[-1], mean.numel()
        L = _L()
        gy = _flat(gy)
        gx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _ws(L.vqw_layernorm_ws_bytes(rows, C), x)
        L.vqw_layernorm_bwd(x, weight, mean, rstd, gy, gx, dgamma, dbeta, ws, ws.numel(), rows, C)
        return gx, dgamma, dbeta, None


def layer_norm(x, weight, bias, eps=1e-5):
    """nn.LayerNorm(C, eps, elementwise_affine=True)(x) over the last axis of any tensor whose trailing dimension is C."""
    return _LayerNorm.apply(x, weight, bias, float(eps))


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = _flat(x)
        y = torch.empty_like(x)
        _L().vqw_gelu_fwd(x, y, x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        _L().vqw_gelu_bwd(x, _flat(gy), gx, x.numel())
        return gx


def gelu(x):
    """nn.GELU() in its exact form, 0.5 x (1 + erf(x / sqrt 2))."""
    return _Gelu.apply(x)


def linear(x, weight, bias=None):
    """F.linear(x, weight, bias) on a (B, T, C) tensor: the 1 x 1 convolution ops.conv2d serves, on the channels-last view
    (B, C, T, 1) of x (the same memory) with the 2-D weight viewed as (out, in, 1, 1).  The parameter stays nn.Linear's 2-D
    weight: the 4-D view is no leaf, so the weight and bias gradients flow through autograd (never the out-of-band route, which
    writes into the .grad of the tensor it is handed) and arrive in weight.grad / bias.grad with the parameters' own shapes."""
    if x.dim() != 3 or weight.dim() != 2:
        raise RuntimeError("linear: expected x (B, T, C) and a 2-D weight, got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
    y = conv2d(x.transpose(1, 2).unsqueeze(-1), weight.view(weight.shape[0], weight.shape[1], 1, 1), bias)
    return y.squeeze(-1).transpose(1, 2)                 # (B, T, out), dense: the convolution's NHWC output


def _heads(q, k, v, n_head, n_unmasked, causal):
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise RuntimeError("causal_attention: q (B, Tq, E) and k, v (B, Tk, E) expected, got %s, %s, %s" % (
            tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    B, Tq, E = q.shape
    if n_head < 1 or E % n_head != 0:
        raise RuntimeError("causal_attention: E=%d is not divisible by n_head=%d" % (E, n_head))
    return B, Tq, k.shape[1], E // n_head, 1.0 / float(E // n_head) ** 0.5, int(bool(causal)), int(n_unmasked)


def _causal_attention_fwd(q, k, v, n_head, n_unmasked, causal, drop=()):
    """drop: () or (p, seed, call, site), the dropout kernels' trailing arguments."""
    _dev(q, k, v)
    q, k, v = _flat(q), _flat(k), _flat(v)
    B, Tq, Tk, hs, scale, causal, nu = _heads(q, k, v, n_head, n_unmasked, causal)
    o = torch.empty_like(q)
    lse = torch.empty(B, n_head, Tq, dtype=torch.float32, device=q.device)
    fwd = _L().vqw_causal_attention_drop_fwd if drop else _L().vqw_causal_attention_fwd
    fwd(q, k, v, o, lse, B, Tq, Tk, n_head, hs, scale, causal, nu, *drop)
    return q, k, v, o, lse, (B, Tq, Tk, hs, scale, causal, nu)


class _CausalAttention(torch.autograd.Function):
    """drop = (p, seed, call, site): dropout on the probabilities, the mask regenerated from it in the backward; (): none."""

    @staticmethod
    def forward(ctx, q, k, v, n_head, n_unmasked, causal, drop):
        q, k, v, o, lse, ctx.cfg = _causal_attention_fwd(q, k, v, n_head, n_unmasked, causal, drop)
        ctx.n_head, ctx.drop = n_head, drop
        ctx.save_for_backward(q, k, v, o, lse)          # the backward recomputes nothing but the scores
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, o, lse = ctx.saved_tensors
        B, Tq, Tk, hs, scale, causal, nu = ctx.cfg
        go = _flat(go)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        d = torch.empty_like(lse)
        bwd = _L().vqw_causal_attention_drop_bwd if ctx.drop else _L().vqw_causal_attention_bwd
        bwd(q, k, v, o, lse, go, d, gq, gk, gv, B, Tq, Tk, ctx.n_head, hs, scale, causal, nu, *ctx.drop)
        return gq, gk, gv, None, None, None, None


def causal_attention(q, k, v, n_head, n_unmasked=0, causal=True, dropout_p=0.0, dropout_key=None):
    """softmax(q k^T / sqrt(hs)) v per head on q (B, Tq, E), k, v (B, Tk, E), E = n_head hs, the heads side by side in the last
    axis (what three nn.Linear projections leave); returns (B, Tq, E).  causal=True (Tq == Tk): query i sees key j iff
    j <= (i < n_unmasked ? n_unmasked - 1 : i) - the reference's tril mask with an all-ones n_unmasked x n_unmasked corner
    (mingpt.py:53-56).  causal=False: no mask, Tq != Tk allowed, forward only (the layer_past route, mingpt.py:71-80).
    dropout_p > 0 with dropout_key = (seed, call, site): dropout on the probabilities (mingpt.py:83) inside the kernels, the mask
    of element (b n_head + h, i, j) regenerated in the backward (Tq == Tk); dropout_p == 0 or no key: the path without it."""
    drop = () if dropout_key is None or dropout_p == 0 else (_drop_p(dropout_p),) + _drop_key(dropout_key)
    return _CausalAttention.apply(q, k, v, int(n_head), int(n_unmasked), bool(causal), drop)


def causal_attention_lse(q, k, v, n_head, n_unmasked=0, causal=True):
    """(output, row log-sum-exp [B, n_head, Tq]) of causal_attention without a tape: for tests and measurement."""
    _, _, _, o, lse, _ = _causal_attention_fwd(q, k, v, int(n_head), int(n_unmasked), bool(causal))
    return o, lse


# ----------------------------------------------------------------------------------------------
# dropout of the GPT prior: counter-based masks (csrc/dropout.h), key = (seed, call, site), nothing saved but the key
# ----------------------------------------------------------------------------------------------
def _drop_p(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout: p=%r must lie in [0, 1)" % (p,))
    return p


def _drop_key(key):
    seed, call, site = (int(v) for v in key)
    if not (-2 ** 63 <= seed < 2 ** 63 and -2 ** 63 <= call < 2 ** 63 and -2 ** 31 <= site < 2 ** 31):
        raise ValueError("dropout: key (seed, call, site) = %r does not fit (long, long, int)" % ((seed, call, site),))
    return seed, call, site


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, key):
        _dev(x)
        x = _flat(x)
        y = torch.empty_like(x)
        _L().vqw_dropout(x, y, x.numel(), p, *key)
        ctx.p, ctx.key = p, key
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _flat(gy)
        gx = torch.empty_like(gy)
        _L().vqw_dropout(gy, gx, gy.numel(), ctx.p, *ctx.key)          # dropout is linear: the same launch on the gradient
        return gx, None, None


class _AddDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, p, key):
        _dev(a, b)
        a, b = _flat(a), _flat(b)
        if a.shape != b.shape:
            raise RuntimeError("add_dropout: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty_like(a)
        _L().vqw_add_dropout(a, b, y, a.numel(), p, *key)
        ctx.p, ctx.key = p, key
        return y

    @staticmethod
    def backward(ctx, gy):
        gb = None
        if ctx.needs_input_grad[1]:
            gy = _flat(gy)
            gb = torch.empty_like(gy)
            _L().vqw_dropout(gy, gb, gy.numel(), ctx.p, *ctx.key)
        return gy, gb, None, None


def dropout(x, p, key):
    """Training-mode nn.Dropout(p)(x) on a dense fp32 tensor under key = (seed, call, site) (Python ints): element e (the linear
    index) is kept iff its draw of csrc/dropout.h is >= round(p 2^32), a kept element is multiplied by float32(1 / (1 - p)).  The
    backward regenerates the mask from the key: nothing is saved."""
    return _Dropout.apply(x, _drop_p(p), _drop_key(key))


def add_dropout(a, b, p, key):
    """a + dropout(b, p, key) in one pass over dense fp32 tensors of one shape."""
    return _AddDropout.apply(a, b, _drop_p(p), _drop_key(key))


def dropout_keep_mask(n, p, key, device="cuda"):
    """The keep mask (n,) torch.bool of an element-wise site, written by the device function the kernels use: for tests and for
    looking at a mask."""
    out = torch.empty(int(n), dtype=torch.uint8, device=device)
    _dev(out)
    _L().vqw_dropout_mask(out, int(n), _drop_p(p), *_drop_key(key))
    return out.bool()


def attention_keep_mask(B, n_head, Tq, Tk, p, key, device="cuda"):
    """The keep mask (B, n_head, Tq, Tk) torch.bool of an attention site (ops.causal_attention's dropout_key)."""
    out = torch.empty(int(B), int(n_head), int(Tq), int(Tk), dtype=torch.uint8, device=device)
    _dev(out)
    _L().vqw_attention_dropout_mask(out, int(B), int(n_head), int(Tq), int(Tk), _drop_p(p), *_drop_key(key))
    return out.bool()


# ----------------------------------------------------------------------------------------------
# the GPT code prior around the blocks (networks/gpt.py): embedding, cross-entropy, top-k sampling
# ----------------------------------------------------------------------------------------------
def _long(t, what):
    if t.dtype != torch.long:
        raise RuntimeError("%s must be torch.long (got %s)" % (what, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, tok, pos, prefix, t0):
        _dev(idx, tok, pos, prefix)
        if prefix is not None and prefix.dim() == 3 and prefix.shape[1] == 0:
            prefix = None
        idx, tok, pos = _long(idx, "embedding: idx"), _flat(tok), _flat(pos)
        if idx.dim() != 2 or tok.dim() != 2 or pos.dim() < 2 or pos.shape[-1] != tok.shape[1] or pos.numel() != pos.shape[-2] * pos.shape[-1]:
            raise RuntimeError("embedding: idx (B, Ti), tok (V, E) and pos ([1,] block_size, E) expected, got %s, %s, %s" % (
                tuple(idx.shape), tuple(tok.shape), tuple(pos.shape)))
        (B, Ti), (V, E), block_size, Te = idx.shape, tok.shape, pos.shape[-2], 0
        if prefix is not None:
            prefix = _flat(prefix)
            if prefix.dim() != 3 or prefix.shape[0] != B or prefix.shape[2] != E:
                raise RuntimeError("embedding: prefix (B, Te, E) = (%d, Te, %d) expected, got %s" % (B, E, tuple(prefix.shape)))
            Te = prefix.shape[1]
        x = torch.empty(B, Te + Ti, E, dtype=torch.float32, device=tok.device)
        _L().vqw_embed_fwd(idx, tok, pos, prefix, x, B, Ti, Te, E, V, block_size, t0)
        ctx.save_for_backward(idx)
        ctx.cfg = (B, Ti, Te, E, V, block_size, t0, tuple(pos.shape))
        return x

    @staticmethod
    def backward(ctx, gx):
        (idx,) = ctx.saved_tensors
        B, Ti, Te, E, V, block_size, t0, pos_shape = ctx.cfg
        gx = _flat(gx)
        gtok = torch.empty(V, E, dtype=torch.float32, device=gx.device)
        gpos = torch.empty(pos_shape, dtype=torch.float32, device=gx.device)
        _L().vqw_embed_bwd(idx, gx, gtok, gpos, B, Ti, Te, E, V, block_size, t0)
        return None, gtok, gpos, (gx[:, :Te] if Te > 0 and ctx.needs_input_grad[3] else None), None


def embedding(idx, tok, pos, prefix=None, t0=0):
    """x[b, t] = (prefix[b, t] if t < Te else tok[idx[b, t - Te]]) + pos[t0 + t]: the input stem of GPT (mingpt.py:177-189) on idx
    (B, Ti) torch.long, tok (V, E), pos (block_size, E) or (1, block_size, E), prefix (B, Te, E) or None (the reference's
    `embeddings=`); returns (B, Te + Ti, E).  t0 is the position offset of the first row (past_length on the cached route).
    Gradients go to tok, pos and prefix.  An index outside [0, V) gives a NaN row and no gradient."""
    return _Embedding.apply(idx, tok, pos, prefix, int(t0))


def _xent_fwd(logits, target, want_mean):
    _dev(logits, target)
    z = _flat(logits)
    if z.dim() < 1 or tuple(target.shape) != tuple(z.shape[:-1]):
        raise RuntimeError("cross_entropy: logits (..., V) and target (...) expected, got %s and %s" % (tuple(logits.shape), tuple(target.shape)))
    target = _long(target, "cross_entropy: target")
    V = z.shape[-1]
    rows = z.numel() // max(V, 1)
    L = _L()
    loss = torch.empty(z.shape[:-1], dtype=torch.float32, device=z.device)
    lse = torch.empty(z.shape[:-1], dtype=torch.float32, device=z.device)
    mean = torch.empty((), dtype=torch.float32, device=z.device) if want_mean else None
    ws = _ws(L.vqw_xent_ws_bytes(rows), z) if want_mean else None
    L.vqw_xent_fwd(z, target, loss, lse, mean, ws, ws.numel() if want_mean else 0, rows, V)
    return z, target, loss, lse, mean


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, want_mean):
        z, target, loss, lse, mean = _xent_fwd(logits, target, want_mean)
        ctx.save_for_backward(z, target, lse)
        ctx.want_mean = want_mean
        return mean if want_mean else loss

    @staticmethod
    def backward(ctx, g):
        z, target, lse = ctx.saved_tensors
        V = z.shape[-1]
        gz = torch.empty_like(z)
        _L().vqw_xent_bwd(z, target, lse, _flat(g), gz, z.numel() // V, V, int(ctx.want_mean))      # g stays on the device
        return gz, None, None


def cross_entropy(logits, target, reduction="mean"):
    """F.cross_entropy over the last axis: logits (..., V), target (...) torch.long -> the mean over all rows (a 0-dim tensor) or,
    reduction='none', the loss per row with the leading shape.  A target outside [0, V) gives NaN in its row (and in the mean)."""
    if reduction not in ("mean", "none"):
        raise ValueError("cross_entropy: reduction must be 'mean' or 'none' (got %r)" % (reduction,))
    return _CrossEntropy.apply(logits, target, reduction == "mean")


def cross_entropy_lse(logits, target):
    """(loss per row, row log-sum-exp), both with the leading shape of logits, without a tape: for tests and measurement."""
    _, _, loss, lse, _ = _xent_fwd(logits, target, False)
    return loss, lse


def _sample_args(name, logits, u):
    _dev(logits, u)
    logits, u = _flat(logits), _flat(u)
    if logits.dim() != 2 or u.dim() != 1 or u.shape[0] != logits.shape[0]:
        raise RuntimeError("%s: logits (B, V) and u (B,) expected, got %s and %s" % (name, tuple(logits.shape), tuple(u.shape)))
    return logits, u, torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)


def sample_topk(logits, u, temperature=1.0, top_k=0):
    """One token per row of logits (B, V): top_k_logits (keep every entry >= the top_k-th largest of logits / temperature; 0, None
    or >= V: no filter), softmax, inverse-CDF sampling with the caller's uniforms u (B,) in [0, 1) - torch.rand with a generator.
    Returns (B,) torch.long.  No random numbers are drawn here: the same u gives the same tokens."""
    logits, u, out = _sample_args("sample_topk", logits, u)
    _L().vqw_sample_topk(logits, u, out, logits.shape[0], logits.shape[1], float(temperature), int(top_k or 0))
    return out


def sample_filtered(logits, u, forced=None, temperature=1.0, top_k=0, top_p=None, return_logp=True):
    """One token per row of logits (B, V), sampled or forced -> (tokens (B,) torch.long, logp (B,) fp32 or None).
    Filter: sample_topk's top-k (0, None or >= V: none), then the nucleus over what it kept: an entry stays iff the mass of the
    kept entries strictly greater than it is <= top_p (top_k_top_p_filtering's rule; ties share one fate; None or >= 1: no
    filter).  Draw: sample_topk's inverse CDF with the caller's uniforms u (B,).  forced (B,) torch.long or None: a row whose entry
    lies in [0, V) takes it (u is not read there), a negative entry draws, an entry >= V draws and makes logp NaN.  logp is the
    token's log-probability under the model's own distribution (temperature 1, no filter).  With forced None and no top_p the
    tokens have sample_topk's bits: the two are one kernel."""
    _dev(forced)
    logits, u, out = _sample_args("sample_filtered", logits, u)
    if forced is not None:
        forced = _long(forced, "sample_filtered: forced")
        if tuple(forced.shape) != tuple(u.shape):
            raise RuntimeError("sample_filtered: forced (B,) = %s expected, got %s" % (tuple(u.shape), tuple(forced.shape)))
    B, V = logits.shape
    logp = torch.empty(B, dtype=torch.float32, device=logits.device) if return_logp else None
    _L().vqw_sample_filtered(logits, u, forced, out, logp, B, V, float(temperature), int(top_k or 0), 1.0 if top_p is None else float(top_p))
    return out, logp


def _guidance_scale(name, scale):
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise ValueError("%s: guidance_scale=%r must be finite and not negative" % (name, scale))
    return scale


def sample_guided(logits, u, scale, forced=None, temperature=1.0, top_k=0, top_p=None, out=None):
    """sample_filtered under classifier-free guidance, in the same kernel: logits (2B, V) - the rows [0, B) conditional (z_c), the
    rows [B, 2B) unconditional (z_u) - u (B,), forced (B,) or None -> (tokens (2B,) torch.long with tokens[B:] == tokens[:B], logp
    (B,), logp_u (B,)).  The filter and the draw see z = fmaf(scale, z_c - z_u, z_u), never written to memory; logp and logp_u are
    the token's log-probabilities under z_c and under z_u (temperature 1, unfiltered): what sample_filtered returns for that row
    with the token forced.  scale: finite, >= 0.  `out`: a (2B,) torch.long buffer to write the tokens into."""
    _dev(logits, u, forced)
    scale = _guidance_scale("sample_guided", scale)
    logits, u = _flat(logits), _flat(u)
    if logits.dim() != 2 or u.dim() != 1 or logits.shape[0] != 2 * u.shape[0] or u.shape[0] < 1:
        raise RuntimeError("sample_guided: logits (2B, V) and u (B,) expected, got %s and %s" % (tuple(logits.shape), tuple(u.shape)))
    B, V = u.shape[0], logits.shape[1]
    if forced is not None:
        forced = _long(forced, "sample_guided: forced")
        if tuple(forced.shape) != (B,):
            raise RuntimeError("sample_guided: forced (B,) = (%d,) expected, got %s" % (B, tuple(forced.shape)))
    if out is None:
        out = torch.empty(2 * B, dtype=torch.long, device=logits.device)
    elif out.dtype != torch.long or tuple(out.shape) != (2 * B,) or not out.is_contiguous() or out.device != logits.device:
        raise RuntimeError("sample_guided: out must be a contiguous (2B,) = (%d,) torch.long tensor on the logits' device" % (2 * B))
    logp = torch.empty(B, dtype=torch.float32, device=logits.device)
    logp_u = torch.empty(B, dtype=torch.float32, device=logits.device)
    _L().vqw_sample_guided(logits, u, forced, out, logp, logp_u, B, V, scale, float(temperature), int(top_k or 0),
                           1.0 if top_p is None else float(top_p))
    return out, logp, logp_u


def paste_cells(image, edit, cellmask):
    """The composite of an edit: out = edit where the latent cell of the pixel is set in cellmask (B, h, w) torch.uint8, else
    image; image and edit (B, C, H, W) fp32 in either memory format, H and W multiples of h and w.  Returns a channels_last
    tensor.  No gradient."""
    _dev(image, edit, cellmask)
    image, edit = nhwc(image.detach()), nhwc(edit.detach())
    if image.shape != edit.shape:
        raise RuntimeError("paste_cells: shape mismatch %s vs %s" % (tuple(image.shape), tuple(edit.shape)))
    N, C, H, W = image.shape
    if cellmask.dtype != torch.uint8 or cellmask.dim() != 3 or cellmask.shape[0] != N:
        raise RuntimeError("paste_cells: cellmask (B, h, w) torch.uint8 with B = %d expected, got %s of %s" % (N, tuple(cellmask.shape), cellmask.dtype))
    h, w = cellmask.shape[1:]
    if h < 1 or w < 1 or H % h or W % w:
        raise RuntimeError("paste_cells: H = %d and W = %d must be multiples of the cell grid %d x %d" % (H, W, h, w))
    out = torch.empty_like(image, memory_format=CL)
    _L().vqw_paste_cells(image, edit, cellmask.contiguous(), out, N, H, W, C, h, w)
    return out


def blend_cells(image, edit, cellmask, levels, recon=None):
    """The seamless composite of an edit: Burt-Adelson multi-band blending over `levels` pyramid levels (csrc/blend.hip; the
    definition is in include/vqwnet_hip.h).  out = image + R_0, where R collapses the Laplacian pyramid of d under the Gaussian
    pyramid of the cell mask; d = edit - image, or edit - recon when recon (the decode of the slice's own codes) is given.
    image, edit, recon (B, C, H, W) fp32 in either memory format, cellmask (B, h, w) torch.uint8, H and W multiples of h, w and
    of 2^levels, 1 <= levels <= 12 (the kernel's argument check refuses the rest).  2 levels launches.  Returns a channels_last
    tensor.  No gradient."""
    _dev(image, edit, cellmask, recon)
    if isinstance(levels, bool) or not isinstance(levels, int):
        raise RuntimeError("blend_cells: levels=%r must be an integer" % (levels,))
    image, edit = nhwc(image.detach()), nhwc(edit.detach())
    if image.shape != edit.shape:
        raise RuntimeError("blend_cells: shape mismatch %s vs %s" % (tuple(image.shape), tuple(edit.shape)))
    if recon is not None:
        recon = nhwc(recon.detach())
        if recon.shape != image.shape:
            raise RuntimeError("blend_cells: shape mismatch %s vs recon %s" % (tuple(image.shape), tuple(recon.shape)))
    N, C, H, W = image.shape
    if cellmask.dtype != torch.uint8 or cellmask.dim() != 3 or cellmask.shape[0] != N:
        raise RuntimeError("blend_cells: cellmask (B, h, w) torch.uint8 with B = %d expected, got %s of %s" % (N, tuple(cellmask.shape), cellmask.dtype))
    h, w = cellmask.shape[1:]
    if h < 1 or w < 1 or H % h or W % w:
        raise RuntimeError("blend_cells: H = %d and W = %d must be multiples of the cell grid %d x %d" % (H, W, h, w))
    floats = int(_L().vqw_blend_cells_workspace(N, H, W, C, levels))       # 0: out of range, and the kernel's check says which
    ws = torch.empty(max(floats, 4), dtype=torch.float32, device=image.device)
    out = torch.empty_like(image, memory_format=CL)
    _L().vqw_blend_cells(image, edit, recon, cellmask.contiguous(), out, ws, ws.numel(), N, H, W, C, h, w, levels)
    return out


# ----------------------------------------------------------------------------------------------
# anomaly detection with the code prior (csrc/detect.hip): forward only, no gradient
# ----------------------------------------------------------------------------------------------
SCORE_BINS = 65536
DETECTION_SCORES = ("auroc", "ap", "best_dice", "best_threshold", "P", "N", "err_free", "reserved")


def gauss_taps(sigma):
    """The K = 2 ceil(3 sigma) + 1 taps exp(-d^2 / 2 sigma^2) of anomaly_map's Gaussian, normalised to sum 1 in double and
    rounded to fp32 (a host tensor); sigma = 0: the single tap 1 (no blur)."""
    import math
    sigma = float(sigma)
    if not sigma >= 0 or math.isinf(sigma):
        raise ValueError("gauss_taps: sigma=%r must be a finite number >= 0" % (sigma,))
    if sigma == 0:
        return torch.ones(1, dtype=torch.float32)
    R = int(math.ceil(3.0 * sigma))
    d = torch.arange(-R, R + 1, dtype=torch.float64)
    t = torch.exp(-d * d / (2.0 * sigma * sigma))
    return (t / t.sum()).float()


_device_taps = {}


def _taps_on_device(sigma, device):
    """gauss_taps(sigma) on the device, copied once per (sigma, device): a call of anomaly_map then has no host-to-device copy."""
    key = (sigma, str(device))
    if key not in _device_taps:
        _device_taps[key] = gauss_taps(sigma).to(device)
    return _device_taps[key]


def anomaly_map(a, b, cellmask=None, sigma=2.0):
    """map = G_sigma(r o U(m)) -> (N, H, W) fp32: r = mean_c |a - b| of a, b (N, C, H, W) fp32 in either memory format; m =
    float(cellmask != 0) for cellmask (N, h, w) torch.uint8 with H, W integer multiples of h, w, U its bilinear up-sampling
    (F.interpolate(mode='bilinear', align_corners=False)); cellmask None: no weight.  G_sigma: the separable Gaussian of
    gauss_taps(sigma) with replicate borders; sigma = 0: no blur.  One kernel; refused by its argument check: a sigma whose
    K = 2 ceil(3 sigma) + 1 exceeds 33 taps, non-integer factors, empty tensors.  No gradient."""
    _dev(a, b, cellmask)
    a, b = nhwc(a.detach()), nhwc(b.detach())
    if a.shape != b.shape:
        raise RuntimeError("anomaly_map: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    N, C, H, W = a.shape
    h = w = 1
    if cellmask is not None:
        if cellmask.dtype != torch.uint8 or cellmask.dim() != 3 or cellmask.shape[0] != N:
            raise RuntimeError("anomaly_map: cellmask (N, h, w) torch.uint8 with N = %d expected, got %s of %s" % (N, tuple(cellmask.shape), cellmask.dtype))
        cellmask = cellmask.contiguous()
        h, w = cellmask.shape[1:]
    taps = _taps_on_device(float(sigma), a.device)
    out = torch.empty((N, H, W), dtype=torch.float32, device=a.device)
    _L().vqw_anomaly_map(a, b, cellmask, taps, out, N, H, W, C, h, w, taps.numel())
    return out


def new_score_histogram(device):
    """(hist (2, 65536) torch.long, err (1,) torch.long), zeroed, for score_histogram to accumulate into."""
    return torch.zeros((2, SCORE_BINS), dtype=torch.long, device=device), torch.zeros(1, dtype=torch.long, device=device)


def score_histogram(scores, labels, hist, err):
    """Adds the scores (any shape, fp32) to hist (2, 65536) torch.long IN PLACE - hist[0] the pixels whose label is 0, hist[1] the
    others - by the key bits(s) >> 15 of a finite s >= 0 (-0 is 0); a NaN, an infinity or a negative score is not binned and
    adds 1 to err (1,) torch.long.  labels: torch.uint8 (or torch.bool) with as many elements.  Returns None."""
    _dev(scores, labels, hist, err)
    scores = _flat(scores.detach()).reshape(-1)
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8) if labels.is_contiguous() else labels.contiguous().view(torch.uint8)
    if labels.dtype != torch.uint8 or labels.numel() != scores.numel():
        raise RuntimeError("score_histogram: labels torch.uint8 with %d elements expected, got %s of %s" % (scores.numel(), tuple(labels.shape), labels.dtype))
    if hist.dtype != torch.long or tuple(hist.shape) != (2, SCORE_BINS) or not hist.is_contiguous():
        raise RuntimeError("score_histogram: hist (2, %d) torch.long, contiguous, expected, got %s of %s" % (SCORE_BINS, tuple(hist.shape), hist.dtype))
    if err.dtype != torch.long or err.numel() != 1:
        raise RuntimeError("score_histogram: err (1,) torch.long expected, got %s of %s" % (tuple(err.shape), err.dtype))
    _L().vqw_score_histogram(scores, labels.contiguous().reshape(-1), hist, err, scores.numel())


def detection_scores(hist, err=None):
    """(8,) float64 on the device from a score histogram: [auroc, ap, best_dice, best_threshold, P, N, err-free flag, 0]
    (DETECTION_SCORES names them; the definitions are vqw_detection_scores' in include/vqwnet_hip.h).  With no positive or no
    negative pixel the first four are NaN.  err: score_histogram's counter (None: the flag is 1).  One launch, no host read."""
    _dev(hist, err)
    if hist.dtype != torch.long or tuple(hist.shape) != (2, SCORE_BINS) or not hist.is_contiguous():
        raise RuntimeError("detection_scores: hist (2, %d) torch.long, contiguous, expected, got %s of %s" % (SCORE_BINS, tuple(hist.shape), hist.dtype))
    if err is not None and (err.dtype != torch.long or err.numel() != 1):
        raise RuntimeError("detection_scores: err (1,) torch.long expected, got %s of %s" % (tuple(err.shape), err.dtype))
    out = torch.empty(8, dtype=torch.float64, device=hist.device)
    _L().vqw_detection_scores(hist, err, out)
    return out


# ----------------------------------------------------------------------------------------------
# lesion-wise detection scores (csrc/components.hip): connected components, their areas, the matching
# ----------------------------------------------------------------------------------------------
LESION_ACC = ("slices", "gt_lesions", "gt_detected", "pred_components", "pred_false", "inter", "pred_pixels", "gt_pixels")


def component_cap(H, W, connectivity=8):
    """The most components an H x W image can hold: ceil(H / 2) ceil(W / 2) under connectivity 8, ceil(H W / 2) under 4."""
    if connectivity not in (4, 8):
        raise RuntimeError("component_cap: connectivity=%r must be 4 or 8" % (connectivity,))
    return ((H + 1) // 2) * ((W + 1) // 2) if connectivity == 8 else (H * W + 1) // 2


def _component_map(name, what, t):
    if t.dtype != torch.int32 or t.dim() != 3:
        raise RuntimeError("%s: %s (N, H, W) torch.int32 expected, got %s of %s" % (name, what, tuple(t.shape), t.dtype))
    return t.contiguous()


def _component_counts(name, what, t, N):
    if t.dtype != torch.int32 or tuple(t.shape) != (N,):
        raise RuntimeError("%s: %s (%d,) torch.int32 expected, got %s of %s" % (name, what, N, tuple(t.shape), t.dtype))
    return t.contiguous()


def label_components(x, threshold=None, connectivity=8, err=None):
    """Connected components of the images x (N, H, W) -> (labels (N, H, W) torch.int32, counts (N,) torch.int32, err (1,)
    torch.int32).  x torch.uint8 (or torch.bool): foreground = non-zero; with `threshold` x is fp32 and foreground = x >= threshold
    (a NaN score is background).  connectivity 4 or 8, per image, never across images.  Background is 0; the components of image
    n are numbered 1..counts[n] in raster order of each component's first pixel (scipy.ndimage.label's numbering).  err is the
    kernels' error word (vqw_label_components in include/vqwnet_hip.h): 0 unless a walk passed its step bound, which no input
    can cause - a result with err != 0 is not to be used; it is left on the device so that the call makes no host read.  With
    `err` given (a (1,) torch.int32 tensor) the bits are ORed into it and it is the one returned: an accumulator keeps one word."""
    _dev(x, err)
    if x.dim() != 3:
        raise RuntimeError("label_components: x (N, H, W) expected, got shape %s" % (tuple(x.shape),))
    if x.numel() == 0:
        raise RuntimeError("label_components: an empty tensor %s is refused" % (tuple(x.shape),))
    if connectivity not in (4, 8):
        raise RuntimeError("label_components: connectivity=%r must be 4 or 8" % (connectivity,))
    mask = scores = None
    if threshold is None:
        if x.dtype == torch.bool:
            x = x.contiguous().view(torch.uint8)
        if x.dtype != torch.uint8:
            raise RuntimeError("label_components: without a threshold x is torch.uint8 (foreground = non-zero), got %s" % x.dtype)
        mask = x.contiguous()
    else:
        if x.dtype != torch.float32:
            raise RuntimeError("label_components: with a threshold x is torch.float32 (foreground = x >= threshold), got %s" % x.dtype)
        threshold = float(threshold)
        if threshold != threshold:
            raise RuntimeError("label_components: the threshold is NaN")
        scores = x.detach().contiguous()
    N, H, W = x.shape
    if N * H * W >= 2 ** 31:
        raise RuntimeError("label_components: N H W = %d must stay below 2^31 (32-bit pixel indices)" % (N * H * W))
    L = _L()
    labels = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    counts = torch.empty(N, dtype=torch.int32, device=x.device)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=x.device)
    elif err.dtype != torch.int32 or err.numel() != 1:
        raise RuntimeError("label_components: err (1,) torch.int32 expected, got %s of %s" % (tuple(err.shape), err.dtype))
    ws = torch.empty(max(int(L.vqw_label_components_ws_ints(N, H, W)), 4), dtype=torch.int32, device=x.device)
    L.vqw_label_components(mask, scores, 0.0 if threshold is None else threshold, labels, counts, err, ws, ws.numel(), N, H, W, connectivity)
    return labels, counts, err


def component_areas(labels, counts, connectivity=8, err=None):
    """(N, cap) torch.int32: entry [n][l - 1] is the pixel count of component l of image n, entries past counts[n] are 0.  cap =
    component_cap(H, W, connectivity), a function of the shape alone: pass the connectivity the labels were made with (4 gives
    the larger cap, which holds either).  A label outside [0, cap] is not counted and sets bit 8 of err (1,) torch.int32 when
    given (label_components' error word).  `counts` is checked for its shape only: the areas follow from the labels."""
    _dev(labels, counts, err)
    labels = _component_map("component_areas", "labels", labels)
    N, H, W = labels.shape
    if labels.numel() == 0:
        raise RuntimeError("component_areas: an empty tensor %s is refused" % (tuple(labels.shape),))
    _component_counts("component_areas", "counts", counts, N)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=labels.device)
    elif err.dtype != torch.int32 or err.numel() != 1:
        raise RuntimeError("component_areas: err (1,) torch.int32 expected, got %s of %s" % (tuple(err.shape), err.dtype))
    cap = component_cap(H, W, connectivity)
    areas = torch.empty((N, cap), dtype=torch.int32, device=labels.device)
    _L().vqw_component_areas(labels, areas, err, N, H, W, cap)
    return areas


def new_lesion_acc(device, k=1):
    """(k, 8) torch.long, zeroed: one row of lesion_match's counters (LESION_ACC names them) per threshold."""
    return torch.zeros((int(k), len(LESION_ACC)), dtype=torch.long, device=device)


def lesion_match(pred_labels, pred_counts, pred_areas, gt_labels, gt_counts, min_size, acc):
    """Adds the matching of predicted against ground-truth components to acc (8,) torch.long IN PLACE (LESION_ACC; the definitions
    are vqw_lesion_match's in include/vqwnet_hip.h): a predicted component is kept when its area is >= min_size; a ground-truth
    component is detected when it shares a pixel with a kept one; a kept one that shares no pixel with the ground truth is false.
    pred_areas: component_areas(pred_labels, pred_counts, ...).  No host read.  Returns None."""
    _dev(pred_labels, pred_counts, pred_areas, gt_labels, gt_counts, acc)
    pred_labels, gt_labels = _component_map("lesion_match", "pred_labels", pred_labels), _component_map("lesion_match", "gt_labels", gt_labels)
    if pred_labels.shape != gt_labels.shape:
        raise RuntimeError("lesion_match: label maps of different shapes: pred_labels %s, gt_labels %s" % (tuple(pred_labels.shape), tuple(gt_labels.shape)))
    N, H, W = pred_labels.shape
    if pred_labels.numel() == 0:
        raise RuntimeError("lesion_match: an empty tensor %s is refused" % (tuple(pred_labels.shape),))
    pred_counts, gt_counts = _component_counts("lesion_match", "pred_counts", pred_counts, N), _component_counts("lesion_match", "gt_counts", gt_counts, N)
    if pred_areas.dtype != torch.int32 or pred_areas.dim() != 2 or pred_areas.shape[0] != N or pred_areas.shape[1] < 1 or not pred_areas.is_contiguous():
        raise RuntimeError("lesion_match: pred_areas (%d, cap) torch.int32, contiguous, expected, got %s of %s" % (N, tuple(pred_areas.shape), pred_areas.dtype))
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1:
        raise RuntimeError("lesion_match: min_size=%r must be an integer >= 1" % (min_size,))
    if acc.dtype != torch.long or tuple(acc.shape) != (len(LESION_ACC),) or not acc.is_contiguous():
        raise RuntimeError("lesion_match: acc (%d,) torch.long, contiguous, expected, got %s of %s" % (len(LESION_ACC), tuple(acc.shape), acc.dtype))
    L = _L()
    pcap, gcap = pred_areas.shape[1], component_cap(H, W, 4)          # the ground truth's connectivity is not known here: 4's cap holds either
    ws = torch.empty(max(int(L.vqw_lesion_match_ws_bytes(N, pcap, gcap)), 16), dtype=torch.uint8, device=acc.device)
    L.vqw_lesion_match(pred_labels, pred_counts, pred_areas, gt_labels, gt_counts, acc, ws, ws.numel(), N, H, W, pcap, gcap, int(min_size))


# ----------------------------------------------------------------------------------------------
# scores of the prior's samples (csrc/sample_scores.hip): feature rows (N, D) fp32, used as fp32(x - shift)
# ----------------------------------------------------------------------------------------------
FEATURE_MAX_D = 2048
KNN_MAX_K = 8


def _feature_rows(name, x, what, D=None):
    _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError("%s: %s (N, D) fp32 with N, D >= 1 expected, got %s of %s" % (name, what, tuple(x.shape), x.dtype))
    if not 1 <= x.shape[1] <= FEATURE_MAX_D:
        raise RuntimeError("%s: D=%d out of [1, %d]" % (name, x.shape[1], FEATURE_MAX_D))
    if D is not None and x.shape[1] != D:
        raise RuntimeError("%s: %s has D=%d, expected %d" % (name, what, x.shape[1], D))
    return x.detach().contiguous()


def _feature_shift(name, shift, D, like):
    if shift is None:
        return None
    _dev(shift)
    if shift.dtype != torch.float32 or tuple(shift.shape) != (D,) or shift.device != like.device:
        raise RuntimeError("%s: shift (%d,) fp32 on %s expected, got %s of %s" % (name, D, like.device, tuple(shift.shape), shift.dtype))
    return shift.detach().contiguous()


def feature_moments(x, sum, outer, shift=None):
    """Adds the moments of the feature rows x (N, D) fp32 IN PLACE: sum (D,) float64 += sum_n y, outer (D, D) float64 += sum_n y
    y^T with y = fp32(x - shift), the products and sums in double, in a fixed order (the same bytes every run), outer exactly
    symmetric.  sum and outer are contiguous float64 tensors the caller zeroed once; shift (D,) fp32 or None.  Returns None.  No
    gradient."""
    x = _feature_rows("feature_moments", x, "x")
    N, D = x.shape
    _dev(sum, outer)
    if sum.dtype != torch.float64 or tuple(sum.shape) != (D,) or not sum.is_contiguous():
        raise RuntimeError("feature_moments: sum (%d,) float64, contiguous, expected, got %s of %s" % (D, tuple(sum.shape), sum.dtype))
    if outer.dtype != torch.float64 or tuple(outer.shape) != (D, D) or not outer.is_contiguous():
        raise RuntimeError("feature_moments: outer (%d, %d) float64, contiguous, expected, got %s of %s" % (D, D, tuple(outer.shape), outer.dtype))
    shift = _feature_shift("feature_moments", shift, D, x)
    L = _L()
    ws = _ws(L.vqw_feature_moments_ws_bytes(N, D), x)
    L.vqw_feature_moments(x, shift, sum, outer, ws, ws.numel(), N, D)


def knn_radius(a, k, shift=None):
    """(N,) fp32: r2[i] = the k-th smallest squared distance from row i of a (N, D) fp32 to the OTHER rows (self is excluded by
    index, so a duplicate of row i counts, at distance exactly 0).  d2 = max(0, |q|^2 + |a|^2 - 2 q.a) over y = fp32(x - shift) on
    the exact-fp32 matrix cores; the N x N distances are never written.  1 <= k <= 8, N >= k + 1.  No gradient."""
    a = _feature_rows("knn_radius", a, "a")
    N, D = a.shape
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("knn_radius: k=%d out of [1, %d]" % (k, KNN_MAX_K))
    if N < k + 1:
        raise ValueError("knn_radius: N=%d must be at least k + 1 = %d (self is excluded)" % (N, k + 1))
    shift = _feature_shift("knn_radius", shift, D, a)
    r2 = torch.empty(N, dtype=torch.float32, device=a.device)
    L = _L()
    ws = _ws(L.vqw_knn_radius_ws_bytes(N), a)
    L.vqw_knn_radius(a, shift, r2, ws, ws.numel(), N, D, k)
    return r2


def ball_counts(q, a, r2, shift=None):
    """(cnt_q (M,), hit_a (N,)) torch.int32 for queries q (M, D), centres a (N, D) and squared radii r2 (N,), all fp32: cnt_q[m] =
    the number of balls i with d2(q_m, a_i) <= r2[i] (inclusive), hit_a[i] = the number of queries inside ball i.  knn_radius's
    distances; a NaN radius contains nobody.  The M x N distances are never written.  No gradient."""
    q = _feature_rows("ball_counts", q, "q")
    M, D = q.shape
    a = _feature_rows("ball_counts", a, "a", D)
    N = a.shape[0]
    _dev(r2)
    if r2.dtype != torch.float32 or tuple(r2.shape) != (N,) or r2.device != a.device or q.device != a.device:
        raise RuntimeError("ball_counts: r2 (%d,) fp32 on the device of q and a expected, got %s of %s" % (N, tuple(r2.shape), r2.dtype))
    r2 = r2.detach().contiguous()
    shift = _feature_shift("ball_counts", shift, D, a)
    cnt_q = torch.empty(M, dtype=torch.int32, device=a.device)
    hit_a = torch.empty(N, dtype=torch.int32, device=a.device)
    L = _L()
    ws = _ws(L.vqw_ball_counts_ws_bytes(M, N), a)
    L.vqw_ball_counts(q, a, r2, shift, cnt_q, hit_a, ws, ws.numel(), M, N, D)
    return cnt_q, hit_a


def prior_tokens(ids, sos, pkeep, vocab_size, u_keep=None, u_rand=None):
    """The transformer's input of a training step of the prior, from the code sequences ids (B, T) torch.long: the start token
    `sos` in front of the sequence shifted right by one (teacher forcing; the target stays `ids`), with taming-transformers'
    pkeep corruption: an entry whose u_keep is not below pkeep is replaced by the uniform code min(V - 1, floor(u_rand V)).
    u_keep, u_rand (B, T) fp32 in [0, 1) - torch.rand with a generator; no random numbers are drawn here.  pkeep >= 1 reads
    neither (both may be None).  Returns (B, T) torch.long.  An entry of ids outside [0, V) is passed through."""
    _dev(ids, u_keep, u_rand)
    ids = _long(ids, "prior_tokens: ids")
    if ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
        raise RuntimeError("prior_tokens: ids (B, T) expected, got %s" % (tuple(ids.shape),))
    if pkeep < 1:
        if u_keep is None or u_rand is None:
            raise RuntimeError("prior_tokens: pkeep=%g below 1 needs u_keep and u_rand" % pkeep)
        u_keep, u_rand = _flat(u_keep), _flat(u_rand)
        if tuple(u_keep.shape) != tuple(ids.shape) or tuple(u_rand.shape) != tuple(ids.shape):
            raise RuntimeError("prior_tokens: u_keep and u_rand of shape %s expected, got %s and %s" % (
                tuple(ids.shape), tuple(u_keep.shape), tuple(u_rand.shape)))
    else:
        u_keep = u_rand = None
    inp = torch.empty_like(ids)
    _L().vqw_prior_tokens(ids, u_keep, u_rand, inp, ids.shape[0], ids.shape[1], int(vocab_size), int(sos), float(pkeep))
    return inp


# ----------------------------------------------------------------------------------------------
# conditioning the code prior on label maps (csrc/cond.hip): label tokens per latent cell, changed cells, the table lookup
# ----------------------------------------------------------------------------------------------
_LABEL_DTYPES = {torch.uint8: 1, torch.int32: 4, torch.long: 8}


def _label_map(name, label, h, w):
    """A label map (B, H, W) or (B, 1, H, W), contiguous, of a dtype in _LABEL_DTYPES -> (B, H, W, element size)."""
    _dev(label)
    if label.dtype not in _LABEL_DTYPES:
        raise RuntimeError("%s: a label map of torch.uint8, torch.int32 or torch.long expected, got %s" % (name, label.dtype))
    if label.dim() == 4 and label.shape[1] == 1:
        shape = (label.shape[0],) + tuple(label.shape[2:])
    elif label.dim() == 3:
        shape = tuple(label.shape)
    else:
        raise RuntimeError("%s: a label map (B, H, W) or (B, 1, H, W) expected, got %s" % (name, tuple(label.shape)))
    if not label.is_contiguous():
        raise RuntimeError("%s: the label map must be contiguous" % name)
    B, H, W = shape
    if h < 1 or w < 1 or B < 1 or H < 1 or W < 1 or H % h or W % w:
        raise RuntimeError("%s: H = %d and W = %d must be multiples of the cell grid %d x %d" % (name, H, W, h, w))
    return B, H, W, _LABEL_DTYPES[label.dtype]


def cell_labels(label, h, w, n_labels, want_purity=False):
    """One conditioning token per latent cell: tokens (B, h, w) torch.long, the label in [0, n_labels) that most pixels of the cell
    carry, from label (B, H, W) or (B, 1, H, W) torch.uint8 / int32 / long, contiguous, H % h == 0 and W % w == 0, 1 <= n_labels
    <= 256.  A tie goes to the smallest label; a pixel outside [0, n_labels) counts for nothing; a cell with no counted pixel gets
    -1 (a NaN row downstream).  want_purity: also (B, h, w) fp32 = float(the winner's count) / float(pixels per cell), 0 for the -1
    cell.  Integer counts: the same bits every run.  No gradient."""
    h, w, n_labels = int(h), int(w), int(n_labels)
    B, H, W, es = _label_map("cell_labels", label, h, w)
    if not 1 <= n_labels <= 256:
        raise RuntimeError("cell_labels: n_labels=%d must lie in [1, 256]" % n_labels)
    tokens = torch.empty((B, h, w), dtype=torch.long, device=label.device)
    purity = torch.empty((B, h, w), dtype=torch.float32, device=label.device) if want_purity else None
    _L().vqw_cell_labels(label, tokens, purity, B, H, W, h, w, n_labels, es)
    return (tokens, purity) if want_purity else tokens


def cells_changed(a, b, h, w):
    """(B, h, w) torch.uint8: 1 iff any pixel of the latent cell differs between the label maps a and b (one dtype, one shape;
    cell_labels' layouts).  No gradient."""
    h, w = int(h), int(w)
    B, H, W, es = _label_map("cells_changed", a, h, w)
    _dev(b)
    if b.dtype != a.dtype or tuple(b.shape) != tuple(a.shape) or not b.is_contiguous():
        raise RuntimeError("cells_changed: two contiguous label maps of one dtype and shape expected, got %s of %s and %s of %s" % (
            tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
    out = torch.empty((B, h, w), dtype=torch.uint8, device=a.device)
    _L().vqw_cells_changed(a, b, out, B, H, W, h, w, es)
    return out


class _EmbeddingLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, table):
        _dev(idx, table)
        idx, table = _long(idx, "embedding_lookup: idx"), _flat(table)
        if idx.dim() != 2 or table.dim() != 2 or idx.numel() < 1:
            raise RuntimeError("embedding_lookup: idx (B, T) and table (L, E) expected, got %s and %s" % (tuple(idx.shape), tuple(table.shape)))
        (B, T), (L, E) = idx.shape, table.shape
        out = torch.empty(B, T, E, dtype=torch.float32, device=table.device)
        _L().vqw_embed_lookup(idx, table, out, B * T, E, L)
        ctx.save_for_backward(idx)
        ctx.cfg = (B, T, E, L)
        return out

    @staticmethod
    def backward(ctx, gx):
        # the one embedding gradient (vqw_embed_bwd: a wave owns a table row, ascending (b, t), no sort, no atomics) with no prefix
        # and T positions; the position sums it writes beside the table's gradient are not used
        (idx,) = ctx.saved_tensors
        B, T, E, L = ctx.cfg
        gx = _flat(gx)
        gtable = torch.empty(L, E, dtype=torch.float32, device=gx.device)
        gpos = torch.empty(T, E, dtype=torch.float32, device=gx.device)
        _L().vqw_embed_bwd(idx, gx, gtable, gpos, B, T, 0, E, L, T, 0)
        return None, gtable


def embedding_lookup(idx, table):
    """table[idx]: idx (B, T) torch.long, table (L, E) fp32 -> (B, T, E), a plain gather with a gradient to table - ops.embedding's
    deterministic one.  An index outside [0, L) gives a NaN row and no gradient."""
    return _EmbeddingLookup.apply(idx, table)


COND_DROP_SITE = -1          # csrc/cond.hip: the dropout site of the condition drop, outside the sites GPT.seed_dropout numbers from 0


class _EmbeddingLookupDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, table, null_index, p, seed, call):
        _dev(idx, table)
        idx, table = _long(idx, "embedding_lookup_drop: idx"), _flat(table)
        if idx.dim() != 2 or table.dim() != 2 or idx.numel() < 1:
            raise RuntimeError("embedding_lookup_drop: idx (B, T) and table (L, E) expected, got %s and %s" % (tuple(idx.shape), tuple(table.shape)))
        (B, T), (L, E) = idx.shape, table.shape
        out = torch.empty(B, T, E, dtype=torch.float32, device=table.device)
        eff = torch.empty(B, T, dtype=torch.long, device=table.device)
        _L().vqw_embed_lookup_drop(idx, table, out, eff, B * T, T, E, L, null_index, p, seed, call)
        ctx.save_for_backward(eff)
        ctx.cfg = (B, T, E, L)
        ctx.mark_non_differentiable(eff)
        return out, eff

    @staticmethod
    def backward(ctx, gx, _geff):
        # embedding_lookup's gradient over the indices actually read: a dropped sample's rows add to the null row
        (eff,) = ctx.saved_tensors
        B, T, E, L = ctx.cfg
        gx = _flat(gx)
        gtable = torch.empty(L, E, dtype=torch.float32, device=gx.device)
        gpos = torch.empty(T, E, dtype=torch.float32, device=gx.device)
        _L().vqw_embed_bwd(eff, gx, gtable, gpos, B, T, 0, E, L, T, 0)
        return None, gtable, None, None, None, None


def embedding_lookup_drop(idx, table, null_index, p, seed, call, return_eff=False):
    """embedding_lookup with the condition dropped per sample: sample b of idx (B, T) reads table[null_index] in all its T rows
    iff the draw of csrc/dropout.h for element b under (seed, call, COND_DROP_SITE) falls below round(p 2^32) - no mask tensor, no
    host read, the same bits every run; p = 0 drops nobody and has embedding_lookup's bits.  The table's gradient runs over the
    indices actually read (return_eff: also returned, (B, T) torch.long).  0 <= p < 1, 0 <= null_index < L."""
    seed, call, _ = _drop_key((seed, call, COND_DROP_SITE))
    null_index = int(null_index)
    if not 0 <= null_index < table.shape[0]:
        raise ValueError("embedding_lookup_drop: null_index=%d must be a row of the table (L = %d)" % (null_index, table.shape[0]))
    out, eff = _EmbeddingLookupDrop.apply(idx, table, null_index, _drop_p(p), seed, call)
    return (out, eff) if return_eff else out


class _EmbeddingCond(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, tok, pos, cidx, ctab, null_index, p, seed, call):
        _dev(idx, tok, pos, cidx, ctab)
        idx, cidx = _long(idx, "embedding_cond: idx"), _long(cidx, "embedding_cond: cidx")
        tok, pos, ctab = _flat(tok), _flat(pos), _flat(ctab)
        if idx.dim() != 2 or tok.dim() != 2 or pos.dim() < 2 or pos.shape[-1] != tok.shape[1] or pos.numel() != pos.shape[-2] * pos.shape[-1]:
            raise RuntimeError("embedding_cond: idx (B, T), tok (V, E) and pos ([1,] block_size, E) expected, got %s, %s, %s" % (
                tuple(idx.shape), tuple(tok.shape), tuple(pos.shape)))
        if tuple(cidx.shape) != tuple(idx.shape) or ctab.dim() != 2 or ctab.shape[1] != tok.shape[1]:
            raise RuntimeError("embedding_cond: cidx (B, T) = %s and ctab (L, E) = (L, %d) expected, got %s and %s" % (
                tuple(idx.shape), tok.shape[1], tuple(cidx.shape), tuple(ctab.shape)))
        (B, T), (V, E), L, block_size = idx.shape, tok.shape, ctab.shape[0], pos.shape[-2]
        x = torch.empty(B, T, E, dtype=torch.float32, device=tok.device)
        eff = torch.empty(B, T, dtype=torch.long, device=tok.device)
        _L().vqw_embed_cond_fwd(idx, tok, pos, cidx, ctab, x, eff, B, T, E, V, L, block_size, null_index, p, seed, call)
        ctx.save_for_backward(idx, eff)
        ctx.cfg = (B, T, E, V, L, block_size, tuple(pos.shape))
        ctx.mark_non_differentiable(eff)
        return x, eff

    @staticmethod
    def backward(ctx, gx, _geff):
        # no kernel of its own: ops.embedding's gradient over idx (no prefix) for tok and pos, embedding_lookup_drop's - the same
        # walk over the indices actually read - for the condition's table; its position sums are not used
        idx, eff = ctx.saved_tensors
        B, T, E, V, L, block_size, pos_shape = ctx.cfg
        gx = _flat(gx)
        gtok = gpos = gctab = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gtok = torch.empty(V, E, dtype=torch.float32, device=gx.device)
            gpos = torch.empty(pos_shape, dtype=torch.float32, device=gx.device)
            _L().vqw_embed_bwd(idx, gx, gtok, gpos, B, T, 0, E, V, block_size, 0)
        if ctx.needs_input_grad[4]:
            gctab = torch.empty(L, E, dtype=torch.float32, device=gx.device)
            scratch = torch.empty(T, E, dtype=torch.float32, device=gx.device)
            _L().vqw_embed_bwd(eff, gx, gctab, scratch, B, T, 0, E, L, T, 0)
        return None, gtok, gpos, None, gctab, None, None, None, None


def embedding_cond(idx, tok, pos, cidx, ctab, null_index=None, drop=None, return_eff=False):
    """x[b, t] = (tok[idx[b, t]] + pos[t]) + ctab[e[b, t]]: ops.embedding with a second table's row ADDED position by position, in
    one pass - the input stem of the label-conditioned MaskedGPT.  idx, cidx (B, T) torch.long, tok (V, E), pos (block_size, E) or
    (1, block_size, E), ctab (L, E); returns (B, T, E).  Two fp32 additions in this order: the bits of ops.embedding(idx, tok, pos) +
    ops.embedding_lookup(cidx, ctab).  drop = (p, seed, call): e is null_index in every row of a dropped sample, decided as
    ops.embedding_lookup_drop decides it (the same function in csrc/cond.hip); None or p = 0 drops nobody and needs no null_index.
    return_eff: also e, (B, T) torch.long.  Gradients go to tok, pos and ctab (ops.embedding's deterministic walks, ctab's over e).
    An idx outside [0, V) or an e outside [0, L) gives a NaN row: that row adds to no row of the table it misses."""
    p, seed, call = (0.0, 0, 0) if drop is None else drop
    p = _drop_p(p)
    seed, call, _ = _drop_key((seed, call, COND_DROP_SITE))
    if p > 0:
        if null_index is None or not 0 <= int(null_index) < ctab.shape[0]:
            raise ValueError("embedding_cond: null_index=%r must be a row of the table (L = %d) when p > 0" % (null_index, ctab.shape[0]))
    x, eff = _EmbeddingCond.apply(idx, tok, pos, cidx, ctab, 0 if null_index is None else int(null_index), p, seed, call)
    return (x, eff) if return_eff else x


# ----------------------------------------------------------------------------------------------
# the bidirectional masked code prior (csrc/masked_prior.hip): the select, the corruption of a step, one decoding iteration.
# No gradient.
# ----------------------------------------------------------------------------------------------
MASK_RATIO_SITE = -2         # csrc/masked_prior.hip: the dropout site of a sample's masking ratio
MASK_KEY_SITE = -3           # and of the keys that order its positions


def _rows(name, t, dtype, shape, what):
    """A contiguous (B, T) tensor of `dtype` (and of `shape`, when given) on the device."""
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError("%s: %s (B, T)%s of %s expected, got %s of %s" % (
            name, what, "" if shape is None else " = %s" % (tuple(shape),), dtype, tuple(t.shape), t.dtype))
    _dev(t)
    return t if t.is_contiguous() else t.contiguous()


def _bytes(name, t, shape, what):
    """A (B, T) mask as torch.uint8 (torch.bool is viewed, not copied)."""
    if t.dtype == torch.bool:
        t = (t if t.is_contiguous() else t.contiguous()).view(torch.uint8)
    return _rows(name, t, torch.uint8, shape, what)


def _counts(name, n, B, device, what):
    """A per-sample count as (B,) torch.int32 on the device: a tensor of B integers, or one Python integer for every sample."""
    if not torch.is_tensor(n):
        return torch.full((B,), int(n), dtype=torch.int32, device=device)
    _dev(n)
    if n.dtype not in (torch.int32, torch.long) or tuple(n.shape) != (B,):
        raise RuntimeError("%s: %s (B,) = (%d,) of torch.int32 expected, got %s of %s" % (name, what, B, tuple(n.shape), n.dtype))
    return n.to(torch.int32).contiguous()


def select_lowest(keys, n, eligible=None):
    """(B, T) torch.uint8: 1 at exactly min(max(n[b], 0), count_b) of the eligible entries of row b of keys (B, T) fp32 - those with
    the smallest (key, position) - and 0 elsewhere.  The keys are compared by the order-preserving integer image of their bits: -0
    lies below +0, the infinities order as numbers.  n: (B,) torch.int32 (or one integer); eligible (B, T) torch.uint8 / bool or
    None (every entry).  Equal keys are taken in ascending position; the same bytes every run."""
    keys = _rows("select_lowest", _flat(keys), torch.float32, None, "keys")
    B, T = keys.shape
    if eligible is not None:
        eligible = _bytes("select_lowest", eligible, keys.shape, "eligible")
    n = _counts("select_lowest", n, B, keys.device, "n")
    out = torch.empty((B, T), dtype=torch.uint8, device=keys.device)
    _L().vqw_select_lowest(keys, eligible, n, out, B, T)
    return out


def mask_tokens(ids, mask_token, seed, call, ratio=None):
    """The corruption of a training step of the masked prior: ids (B, T) torch.long -> (inp (B, T) torch.long with mask_token at
    the masked positions, masked (B, T) torch.uint8, n (B,) torch.int32, the masked count per sample).  Sample b masks n_b =
    clamp(ceil(cos(pi/2 u_b) T), 1, T) positions, u_b the draw of csrc/dropout.h for element b under (seed, call, MASK_RATIO_SITE)
    over 2^32; the positions are the n_b smallest (draw of element b T + t under MASK_KEY_SITE, t): exactly n_b.  ratio in (0, 1]
    replaces the cosine for every sample (validation).  No mask tensor, no host read: a function of (seed, call) alone."""
    if ratio is not None and not 0.0 < float(ratio) <= 1.0:
        raise ValueError("mask_tokens: ratio=%r must lie in (0, 1] (None: the cosine schedule)" % (ratio,))
    seed, call, _ = _drop_key((seed, call, MASK_KEY_SITE))
    ids = _rows("mask_tokens", ids, torch.long, None, "ids")
    B, T = ids.shape
    inp = torch.empty_like(ids)
    masked = torch.empty((B, T), dtype=torch.uint8, device=ids.device)
    n = torch.empty(B, dtype=torch.int32, device=ids.device)
    _L().vqw_mask_tokens(ids, inp, masked, n, B, T, int(mask_token), 0.0 if ratio is None else float(ratio), seed, call)
    return inp, masked, n


def unmask_step(tokens, logp, masked, m0, gamma, tau, mask_token, u=None, fixed_logp=None, return_conf=False):
    """One iteration of parallel decoding, one launch: tokens (B, T) torch.long and logp (B, T) fp32 - sample_filtered's output over
    all B T rows, the known positions forced - masked (B, T) torch.uint8 / bool, m0 (B,) torch.int32: the masked count when
    decoding began.  Per sample n_keep = 0 if gamma <= 0 else max(0, min(cur - 1, floor(gamma m0))) of the cur masked positions
    stay masked: those of lowest (confidence, position), confidence = logp + tau g, g the Gumbel noise of u (B, T) fp32 in [0, 1);
    tau = 0: logp itself and u may be None.  Returns (ids (B, T) with mask_token where still masked, masked (B, T) torch.uint8,
    fixed_logp (B, T)) and, return_conf, the confidences (+inf where nothing was masked).  fixed_logp is updated IN PLACE when
    given - logp where a position turns from masked to fixed, untouched elsewhere - else it starts from zeros."""
    tokens = _rows("unmask_step", tokens, torch.long, None, "tokens")
    B, T = tokens.shape
    logp = _rows("unmask_step", _flat(logp), torch.float32, (B, T), "logp")
    masked = _bytes("unmask_step", masked, (B, T), "masked")
    gamma, tau = float(gamma), float(tau)
    if u is not None:
        u = _rows("unmask_step", _flat(u), torch.float32, (B, T), "u")
    elif tau != 0.0:
        raise RuntimeError("unmask_step: tau=%g needs the uniforms u (only tau = 0 reads none)" % tau)
    m0 = _counts("unmask_step", m0, B, tokens.device, "m0")
    if fixed_logp is None:
        fixed_logp = torch.zeros((B, T), dtype=torch.float32, device=tokens.device)
    else:
        _dev(fixed_logp)
        if fixed_logp.dtype != torch.float32 or tuple(fixed_logp.shape) != (B, T) or not fixed_logp.is_contiguous():
            raise RuntimeError("unmask_step: fixed_logp (B, T) = %s fp32, contiguous, expected (it is updated in place), got %s of %s" % (
                (B, T), tuple(fixed_logp.shape), fixed_logp.dtype))
    ids_out = torch.empty_like(tokens)
    masked_out = torch.empty((B, T), dtype=torch.uint8, device=tokens.device)
    conf = torch.empty((B, T), dtype=torch.float32, device=tokens.device) if return_conf else None
    _L().vqw_unmask_step(tokens, logp, masked, u, m0, ids_out, masked_out, fixed_logp, conf, B, T, gamma, tau, int(mask_token))
    return (ids_out, masked_out, fixed_logp, conf) if return_conf else (ids_out, masked_out, fixed_logp)


# ----------------------------------------------------------------------------------------------
# the pseudo-likelihood map of the masked code prior (csrc/pseudo_nll.hip; MaskedGPT.pseudo_nll): the lattice's inputs and the
# gathering LayerNorm.  No gradient.
# ----------------------------------------------------------------------------------------------
def _lattice(name, grid, stride, s0, ns):
    """(h, w, sy, sx, s0, ns) as integers; the kernels refuse what is out of range, with a message that names it."""
    try:
        (h, w), (sy, sx) = (int(v) for v in grid), (int(v) for v in stride)
    except (TypeError, ValueError):
        raise ValueError("%s: grid=%r and stride=%r must be pairs of integers" % (name, grid, stride)) from None
    return h, w, sy, sx, int(s0), int(ns)


def lattice_inputs(ids, grid, stride, s0, ns, mask_token):
    """The inputs of the passes [s0, s0 + ns) of a pseudo-likelihood map: ids (B, T) torch.long, T = h w of grid = (h, w) ->
    (B ns, T) torch.long, row b ns + (s - s0) = ids[b] with mask_token at every position of group s - position t = y w + x
    belongs to group (y mod sy) sx + (x mod sx) of the S = sy sx groups of stride = (sy, sx).  One streaming launch; no mask
    tensor, no host read.  1 <= sy <= h, 1 <= sx <= w, 0 <= s0, ns >= 1, s0 + ns <= S, mask_token >= 0."""
    h, w, sy, sx, s0, ns = _lattice("lattice_inputs", grid, stride, s0, ns)
    ids = _rows("lattice_inputs", ids, torch.long, None, "ids")
    B, T = ids.shape
    if T != h * w:
        raise RuntimeError("lattice_inputs: ids of T = h w = %d codes expected for the grid %d x %d, got %d" % (h * w, h, w, T))
    inp = torch.empty((B * max(ns, 0), T), dtype=torch.long, device=ids.device)
    _L().vqw_lattice_inputs(ids, inp, B, h, w, sy, sx, s0, ns, int(mask_token))
    return inp


def lattice_gather_ln(x, weight, bias, y, grid, stride, s0, ns, eps=1e-5):
    """The rows of a chunk of passes that a pseudo-likelihood map reads, normalised: x (B ns, T, E) fp32, the trunk's output of
    lattice_inputs' rows in front of ln_f; y (B, T, E) fp32, contiguous, updated IN PLACE and returned: for every (b, t) whose
    group g lies in [s0, s0 + ns), y[b, t] = layer_norm(x[b ns + g - s0, t]) - ops.layer_norm's bits on that row - and every other
    row of y is left untouched, so successive chunks fill one y.  Forward only."""
    _no_grad("lattice_gather_ln", x, weight, bias, y)
    h, w, sy, sx, s0, ns = _lattice("lattice_gather_ln", grid, stride, s0, ns)
    _dev(x, weight, bias, y)
    x, weight, bias = _flat(x), _flat(weight), _flat(bias)
    T = h * w
    if y.dim() != 3 or y.dtype != torch.float32 or not y.is_contiguous() or y.shape[1] != T:
        raise RuntimeError("lattice_gather_ln: y (B, T = %d, E) fp32, contiguous, expected (it is updated in place), got %s of %s" % (
            T, tuple(y.shape), y.dtype))
    B, _, E = y.shape
    if x.dtype != torch.float32 or tuple(x.shape) != (B * ns, T, E):
        raise RuntimeError("lattice_gather_ln: x (B ns, T, E) = %s fp32 expected, got %s of %s" % ((B * ns, T, E), tuple(x.shape), x.dtype))
    if weight.numel() != E or bias.numel() != E:
        raise RuntimeError("lattice_gather_ln: weight / bias of %d / %d elements for a trailing dimension of %d" % (weight.numel(), bias.numel(), E))
    _L().vqw_lattice_gather_ln(x, weight, bias, y, B, h, w, E, sy, sx, s0, ns, float(eps))
    return y


# ----------------------------------------------------------------------------------------------
# cached generation (networks/gpt.py GPT.decode_step / generate): the decode kernels.  Forward only.
# ----------------------------------------------------------------------------------------------
def _no_grad(name, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError("%s is forward only: call it under torch.no_grad() (an argument requires a gradient)" % name)


def dec_linear(x, weight, bias=None, ln=None, gelu=False, residual=None, out=None, out_col=0):
    """act(LN?(x) weight^T + bias) (+ residual) on x (M, K) - M the batch of a decode step - with nn.Linear's weight (N, K), in one
    weight-bandwidth-bound launch.  ln: (gamma, beta, eps) of a LayerNorm applied to the rows of x first, or None; gelu: the exact
    erf GELU; residual (M, N), which may be `out` itself.  Returns (M, N); with out= (M, ld), rows contiguous, the result goes
    to out[:, out_col:out_col + N] - nothing else of `out` is touched - and `out` is returned.  Forward only."""
    gamma, beta, eps = ln if ln is not None else (None, None, 1e-5)
    _dev(x, weight, bias, gamma, beta, residual, out)
    _no_grad("dec_linear", x, weight, bias, gamma, beta, residual)
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise RuntimeError("dec_linear: x (M, K) and weight (N, K) expected, got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
    (M, K), N = x.shape, weight.shape[0]
    x, weight = _flat(x.detach()), _flat(weight.detach())
    bias, gamma, beta, residual = (None if t is None else t.detach() for t in (bias, gamma, beta, residual))
    for t, n, what in ((bias, N, "bias (N,)"), (gamma, K, "ln gamma (K,)"), (beta, K, "ln beta (K,)")):
        if t is not None and (t.dim() != 1 or t.shape[0] != n or not t.is_contiguous()):
            raise RuntimeError("dec_linear: a contiguous %s expected, got %s" % (what, tuple(t.shape)))
    if residual is not None and (tuple(residual.shape) != (M, N) or not residual.is_contiguous()):
        raise RuntimeError("dec_linear: a contiguous residual (M, N) = (%d, %d) expected, got %s" % (M, N, tuple(residual.shape)))
    if out is None:
        out, out_col = torch.empty(M, N, dtype=torch.float32, device=x.device), 0
    elif out.dim() != 2 or out.shape[0] != M or out.stride(1) != 1 or out_col < 0 or out_col + N > out.shape[1] or out.dtype != torch.float32:
        raise RuntimeError("dec_linear: out (M, ld) fp32 with contiguous rows and out_col + N <= ld expected, got %s (strides %s), out_col=%d, N=%d" % (
            tuple(out.shape), out.stride(), out_col, N))
    _L().vqw_dec_linear(x, weight, bias, gamma, beta, residual, out, M, K, N, out.stride(0) if M > 1 else max(out.stride(0), out.shape[1]),
                        int(out_col), int(bool(gelu)), float(eps))
    return out


def dec_attention(q, k_cache, v_cache, Tk, n_head):
    """softmax(q k^T / sqrt(hs)) v per head for ONE query row per batch row: q (B, E), k_cache, v_cache (B, capacity, E) contiguous -
    a plane of the KV cache, the heads side by side in the last axis - against the cache rows [0, Tk); no mask (the layer_past
    route).  Rows at or beyond Tk are never read.  Returns (B, E).  Forward only."""
    _dev(q, k_cache, v_cache)
    _no_grad("dec_attention", q, k_cache, v_cache)
    if q.dim() != 2 or k_cache.dim() != 3 or k_cache.shape != v_cache.shape or k_cache.shape[0] != q.shape[0] or k_cache.shape[2] != q.shape[1]:
        raise RuntimeError("dec_attention: q (B, E) and k_cache, v_cache (B, capacity, E) expected, got %s, %s, %s" % (
            tuple(q.shape), tuple(k_cache.shape), tuple(v_cache.shape)))
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise RuntimeError("dec_attention: the cache planes must be contiguous")
    (B, E), capacity = q.shape, k_cache.shape[1]
    if n_head < 1 or E % n_head != 0:
        raise RuntimeError("dec_attention: E=%d is not divisible by n_head=%d" % (E, n_head))
    hs = E // n_head
    q = _flat(q.detach())
    o = torch.empty_like(q)
    _L().vqw_dec_attention(q, k_cache.detach(), v_cache.detach(), o, B, int(Tk), capacity, int(n_head), hs, 1.0 / float(hs) ** 0.5)
    return o


def gpt_decode_pack_floats(n_layer, E, V):
    """Floats of the packed-weights buffer of gpt_decode_step (the layout is in include/vqwnet_hip.h)."""
    return int(_L().vqw_gpt_decode_pack_floats(int(n_layer), int(E), int(V)))


def gpt_decode_ws_floats(B, E, V):
    """Floats of the activations workspace of gpt_decode_step."""
    return int(_L().vqw_gpt_decode_ws_bytes(int(B), int(E), int(V))) // 4


def gpt_decode_step(packed, tok, pos, idx, kv, logits, ws, t, n_head, eps=1e-5):
    """One decode step of the GPT in one host call (2 + 5 n_layer launches from C): the token idx (B,) torch.long of every row at
    position t, behind the cache kv (n_layer, 2, B, capacity, E) whose rows [0, t) hold the past; row t of every plane is written,
    logits (B, V) are written and returned.  packed: the weights (networks.gpt.pack_decode_weights), tok (V, E), pos ([1,]
    block_size, E): the embedding tables, ws: gpt_decode_ws_floats(B, E, V) floats.  Forward only."""
    _dev(packed, tok, pos, idx, kv, logits, ws)
    _no_grad("gpt_decode_step", packed, tok, pos)
    if kv.dim() != 5 or kv.shape[1] != 2 or tok.dim() != 2 or tuple(logits.shape) != (kv.shape[2], tok.shape[0]) or kv.shape[4] != tok.shape[1]:
        raise RuntimeError("gpt_decode_step: kv (n_layer, 2, B, capacity, E), tok (V, E) and logits (B, V) expected, got %s, %s, %s" % (
            tuple(kv.shape), tuple(tok.shape), tuple(logits.shape)))
    n_layer, _, B, capacity, E = kv.shape
    V = tok.shape[0]
    idx = _long(idx, "gpt_decode_step: idx")
    if idx.numel() != B:
        raise RuntimeError("gpt_decode_step: one token per row expected, idx of shape %s for B=%d" % (tuple(idx.shape), B))
    if pos.dim() < 2 or pos.shape[-1] != E or pos.numel() != pos.shape[-2] * E:
        raise RuntimeError("gpt_decode_step: pos ([1,] block_size, E) expected, got %s" % (tuple(pos.shape),))
    for t_, what in ((packed, "packed"), (kv, "kv"), (logits, "logits"), (ws, "ws"), (tok, "tok"), (pos, "pos")):
        if t_.dtype != torch.float32 or not t_.is_contiguous():
            raise RuntimeError("gpt_decode_step: %s must be a contiguous fp32 tensor" % what)
    if n_head < 1 or E % n_head != 0:
        raise RuntimeError("gpt_decode_step: E=%d is not divisible by n_head=%d" % (E, n_head))
    need = gpt_decode_pack_floats(n_layer, E, V)
    if packed.numel() < need:
        raise RuntimeError("gpt_decode_step: packed weights of %d floats, %d needed" % (packed.numel(), need))
    _L().vqw_gpt_decode_step(packed, tok.detach(), pos.detach(), idx, kv, logits, ws, ws.numel() * 4, B, int(t), capacity, n_layer, int(n_head), E,
                             V, pos.shape[-2], float(eps))
    return logits


class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = nhwc(x)
        N, C, H, W = x.shape
        y = empty_nhwc(N, C, H // 2, W // 2, x)
        _L().vqw_maxpool2_fwd(x, y, N, H, W, C)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        N, C, H, W = x.shape
        gy = nhwc(gy)
        gx = torch.empty_like(x, memory_format=CL)
        _L().vqw_maxpool2_bwd(x, gy, None, gx, N, H, W, C)
        return gx


def maxpool2(x):
    return _MaxPool2.apply(x)


class _ResTail(torch.autograd.Function):
    """out = ReLU(a + b); pooled = MaxPool2d(2)(out) as ONE autograd node (blocks.py:29-36).  `out` has two consumers (the
    pooling and the skip connection): as separate nodes their gradients meet in autograd's add, then pass the ReLU mask —
    three kernels over full-resolution tensors; here one (vqw_res_tail_bwd)."""

    @staticmethod
    def forward(ctx, a, b):
        _dev(a, b)
        a, b = nhwc(a), nhwc(b)
        if a.shape != b.shape:
            raise RuntimeError("res_tail: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        N, C, H, W = a.shape
        L = _L()
        out = torch.empty_like(a, memory_format=CL)
        pooled = empty_nhwc(N, C, H // 2, W // 2, a)
        L.vqw_res_tail_fwd(a, b, out, pooled, N, H, W, C)
        ctx.save_for_backward(out)
        ctx.set_materialize_grads(False)       # an unused output's gradient arrives as None (the kernel takes a null pointer), not as a zero fill
        return pooled, out

    @staticmethod
    def backward(ctx, g_pooled, g_out):
        if g_pooled is None and g_out is None:
            return None, None
        (out,) = ctx.saved_tensors
        N, C, H, W = out.shape
        gp = nhwc(g_pooled) if g_pooled is not None else None
        go = nhwc(g_out) if g_out is not None else None
        gx = torch.empty_like(out, memory_format=CL)
        _L().vqw_res_tail_bwd(out, gp, go, gx, N, H, W, C)
        return gx, gx


RES_TAIL_BWD_FUSED = os.environ.get("VQW_RES_TAIL_BWD_FUSED", "1") != "0"      # 0: vqw_res_tail_bwd, then vqw_inorm_bwd_pair (A/B)


class _ResTailNorm(torch.autograd.Function):
    """ResBlock tail on the RAW outputs of its two conv branches (blocks.py:25-36):
    a = ReLU(InstanceNorm(x2)), b = InstanceNorm(xid), out = ReLU(a + b), pooled = MaxPool2d(2)(out).
    The kernel normalises while it reads, so the two apply passes of the norms disappear; x2's statistics come from its
    convolution's epilogue partials when available.  Backward = the tail's single kernel, then the two norms' backward."""

    @staticmethod
    def forward(ctx, x2, xid, eps, part2, partid=None):
        _dev(x2, xid)
        x2, xid = nhwc(x2), nhwc(xid)
        if x2.shape != xid.shape:
            raise RuntimeError("res_tail_norm: shape mismatch %s vs %s" % (tuple(x2.shape), tuple(xid.shape)))
        N, C, H, W = x2.shape
        L = _L()
        if part2 is not None and partid is not None:      # both norms' statistics from their convolutions' partials: one launch
            mr2 = torch.empty(N * C * 2, dtype=torch.float32, device=x2.device)
            mrid = torch.empty(N * C * 2, dtype=torch.float32, device=x2.device)
            L.vqw_inorm_stats_parts2(part2, part2.numel() // (N * C * 2), mr2, partid,
                                     partid.numel() // (N * C * 2), mrid, N, H * W, C, eps)
        else:
            mr2 = _mean_rstd(x2, part2, eps)
            mrid = _mean_rstd(xid, partid, eps)
        out = torch.empty_like(x2, memory_format=CL)
        pooled = empty_nhwc(N, C, H // 2, W // 2, x2)
        L.vqw_res_tail_norm_fwd(x2, mr2, xid, mrid, out, pooled, N, H, W, C)
        ctx.save_for_backward(x2, xid, mr2, mrid, out)
        ctx.set_materialize_grads(False)
        return pooled, out

    @staticmethod
    def backward(ctx, g_pooled, g_out):
        if g_pooled is None and g_out is None:
            return None, None, None, None, None
        x2, xid, mr2, mrid, out = ctx.saved_tensors
        N, C, H, W = out.shape
        L = _L()
        gp = nhwc(g_pooled) if g_pooled is not None else None
        go = nhwc(g_out) if g_out is not None else None
        g = torch.empty_like(out, memory_format=CL)
        if RES_TAIL_BWD_FUSED and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and not (C & 3):
            # the tail's backward and both norms' backward sums in one pass over (out, gradients, x2, xid); g is written for the
            # apply pass only
            gx2 = torch.empty_like(x2, memory_format=CL)
            gxid = torch.empty_like(xid, memory_format=CL)
            ws = _ws(2 * L.vqw_plane_ws_bytes(N, C, H * W), x2)
            L.vqw_res_tail_bwd_pair(out, gp, go, x2, mr2, xid, mrid, g, gx2, gxid, ws, ws.numel(), N, H, W, C)
            return gx2, gxid, None, None, None
        L.vqw_res_tail_bwd(out, gp, go, g, N, H, W, C)
        gx2 = gxid = None
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:      # both norms' backward, common gradient read once
            gx2 = torch.empty_like(x2, memory_format=CL)
            gxid = torch.empty_like(xid, memory_format=CL)
            ws = _ws(2 * L.vqw_plane_ws_bytes(N, C, H * W), x2)
            L.vqw_inorm_bwd_pair(x2, mr2, xid, mrid, g, gx2, gxid, ws, ws.numel(), N, H * W, C)
            return gx2, gxid, None, None, None
        if ctx.needs_input_grad[0]:
            gx2 = _inorm_bwd(x2, mr2, g, True)
        if ctx.needs_input_grad[1]:
            gxid = _inorm_bwd(xid, mrid, g, False)
        return gx2, gxid, None, None, None


def res_tail_norm(x2, xid, eps=1e-5, part2=None, partid=None):
    """(pooled, out) of the ResBlock tail from the raw conv outputs x2 (main branch, norm + ReLU) and xid (1x1 branch,
    norm only); None when the shape needs the separate operators (odd sizes / channel counts)."""
    N, C, H, W = x2.shape
    if (H | W) & 1 or C & 3:
        return None
    return _ResTailNorm.apply(x2, xid, float(eps), part2, partid)


def res_tail(a, b):
    """(MaxPool2d(2)(ReLU(a + b)), ReLU(a + b)); falls back to the separate operators for odd sizes / channel counts."""
    N, C, H, W = a.shape
    if (H | W) & 1 or C & 3:
        out = add(a, b, relu=True)
        return maxpool2(out), out
    return _ResTail.apply(a, b)


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = nhwc(x)
        y = torch.empty_like(x, memory_format=CL)
        _L().vqw_tanh_fwd(x, y, x.numel())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = nhwc(gy)
        gx = torch.empty_like(y, memory_format=CL)
        _L().vqw_tanh_bwd(y, gy, gx, y.numel())
        return gx


def tanh(x):
    return _Tanh.apply(x)


def affine_(x, scale, shift):
    """In-place x*scale+shift (utils norm/denorm, utils/__init__.py:81-92)."""
    _dev(x)
    if not (x.is_contiguous() or x.is_contiguous(memory_format=CL)):
        raise RuntimeError("affine_: tensor must be dense")
    _L().vqw_affine(x, x, float(scale), float(shift), x.numel())
    return x


class _Mse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _dev(a, b)
        a, b = nhwc(a), nhwc(b)
        if a.shape != b.shape:
            raise RuntimeError("mse_loss: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        L = _L()
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = _ws(L.vqw_reduce_ws_bytes(a.numel()), a)
        L.vqw_mse_fwd(a, b, out, ws, ws.numel(), a.numel())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = torch.empty_like(a, memory_format=CL)
        _L().vqw_mse_bwd(a, b, g, ga, a.numel())
        return ga, None


def mse_loss(a, b):
    """F.mse_loss(a, b, reduction='mean'); gradient flows to `a` only (targets are data)."""
    return _Mse.apply(a, b.detach())


class _WindowMse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha, beta, lo, hi):
        _dev(a, b)
        a, b = nhwc(a), nhwc(b)
        if a.shape != b.shape:
            raise RuntimeError("window_mse_loss: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        L = _L()
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = _ws(L.vqw_reduce_ws_bytes(a.numel()), a)
        L.vqw_window_mse_fwd(a, b, out, ws, ws.numel(), a.numel(), alpha, beta, lo, hi)
        ctx.save_for_backward(a, b)
        ctx.win = (alpha, beta, lo, hi)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a, memory_format=CL)
        _L().vqw_window_mse_bwd(a, b, g.contiguous(), ga, a.numel(), *ctx.win)
        return ga, None, None, None, None, None


F32_MAX = 3.4028234663852886e38           # the largest finite float32 (prints as 3.4028235e38)


def window_map(dataset_window, target_window, clamp=True):
    """(alpha, beta, lo, hi) of w(x) = normalize(denormalize(x, dataset window), target window) for x in the dataset's
    normalised units (utils/__init__.py:17-51 as used by trainers/base.py:290-314); windows are (width, center, scale).
    clamp=False: the same alpha and beta with lo, hi = -/+ the largest finite float32 - the pure affine map of the
    reference's `t_normalize` (utils/__init__.py:30-40, whose clamp is commented out).  The bounds stay finite, so no kernel
    meets an infinity and the "strictly inside (lo, hi)" gradient rule passes every finite value."""
    w0, c0, s0 = dataset_window
    w1, c1, s1 = target_window
    vmax0, vmin0 = c0 + w0 // 2, c0 - w0 // 2
    vmax1, vmin1 = c1 + w1 // 2, c1 - w1 // 2
    # hu = (x / s0 + 0.5) * (vmax0 - vmin0) + vmin0 ;  y = ((clip(hu) - vmin1) / (vmax1 - vmin1) - 0.5) * s1
    a_hu, b_hu = (vmax0 - vmin0) / s0, 0.5 * (vmax0 - vmin0) + vmin0
    k = s1 / (vmax1 - vmin1)
    alpha, beta = a_hu * k, (b_hu - vmin1) * k - 0.5 * s1
    if not clamp:
        return float(alpha), float(beta), -F32_MAX, F32_MAX
    return float(alpha), float(beta), float(-0.5 * s1), float(0.5 * s1)


def window_mse_loss(a, b, dataset_window, target_window, clamp=True):
    """F.mse_loss(to_window(a), to_window(b)): the lung / mediastinal terms of the multi-window reconstruction loss."""
    return _WindowMse.apply(a, b.detach(), *window_map(dataset_window, target_window, clamp=clamp))


_twiddles = {}


def _twiddle_table(n, like):
    """(cos, sin)(2 pi m / n) / sqrt(n), m < n, of the DFTs behind frequency_loss: built once per (device, n), the first
    time a side is seen (a one-time set-up cost outside the steady-state step)."""
    key = (like.device, n)
    tw = _twiddles.get(key)
    if tw is None:
        tw = torch.empty(2 * n, dtype=torch.float32, device=like.device)
        _L().vqw_freq_twiddles(tw, n)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()    # later calls may read it from another stream
        _twiddles[key] = tw
    return tw


class _FreqLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, alpha, pf, log_matrix, batch_matrix, loss_weight, win):
        _dev(pred, target)
        pred, target = nhwc(pred), nhwc(target)
        if pred.shape != target.shape:
            raise RuntimeError("frequency_loss: shape mismatch %s vs %s" % (tuple(pred.shape), tuple(target.shape)))
        N, C, H, W = pred.shape
        if pf < 1 or H % pf or W % pf:
            raise RuntimeError("frequency_loss: H=%d and W=%d must be divisible by patch_factor=%d" % (H, W, pf))
        if not alpha >= 0.0:
            raise RuntimeError("frequency_loss: alpha must be >= 0 (got %r)" % (alpha,))
        L = _L()
        tw_h, tw_w = _twiddle_table(H // pf, pred), _twiddle_table(W // pf, pred)
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = _ws(L.vqw_freq_loss_ws_bytes(N, C, H, W, pf), pred)        # D and the folded maxima, kept for backward
        wargs = (1,) + tuple(float(v) for v in win) if win is not None else (0, 1.0, 0.0, 0.0, 0.0)
        ctx.args = (N, C, H, W, pf, float(alpha), int(bool(log_matrix)), float(loss_weight)) + wargs
        L.vqw_freq_loss_fwd(pred, target, tw_h, tw_w, out, ws, ws.numel(), N, C, H, W, pf, float(alpha),
                            int(bool(log_matrix)), int(bool(batch_matrix)), float(loss_weight), *wargs)
        ctx.save_for_backward(pred, target, tw_h, tw_w, ws)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, target, tw_h, tw_w, ws = ctx.saved_tensors
        gp = torch.empty_like(pred, memory_format=CL) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(target, memory_format=CL) if ctx.needs_input_grad[1] else None
        if gp is None and gt is None:
            return (None,) * 8
        _L().vqw_freq_loss_bwd(pred, target, tw_h, tw_w, g.contiguous(), gp, gt, ws, ws.numel(), *ctx.args)
        return gp, gt, None, None, None, None, None, None


def frequency_loss(pred, target, alpha=1.0, patch_factor=1, log_matrix=False, batch_matrix=False, loss_weight=1.0,
                   window=None):
    """Focal frequency loss (focal-frequency-loss 0.3.0, FocalFrequencyLoss without ave_spectrum / matrix):
    loss_weight * mean(w |fft2(pred - target)|^2) over the patch_factor^2 patches of every (n, c) plane, with the spectrum
    weight w = |D|^alpha (log(. + 1) with log_matrix) normalised by its max per plane (over everything with batch_matrix),
    detached.  window = (alpha, beta, lo, hi) of `window_map`: both images are re-windowed inside the kernel first.
    Gradients flow to both inputs (target's is the negation of pred's, masked by its own window clamp)."""
    if window is not None and len(window) != 4:
        raise RuntimeError("frequency_loss: window must be the (alpha, beta, lo, hi) of window_map")
    return _FreqLoss.apply(pred, target, float(alpha), int(patch_factor), bool(log_matrix), bool(batch_matrix),
                           float(loss_weight), None if window is None else tuple(window))


# out[] slots of vqw_recon_metrics (csrc/metrics.hip)
# ----------------------------------------------------------------------------------------------
# VGG perceptual loss (functions/perceptual_loss.py: VGGLoss(conv_index='22') = vgg19.features[:8])
# ----------------------------------------------------------------------------------------------
_IDENTITY_WINDOW = (1.0, 0.0, float("-inf"), float("inf"))
_window_tables = {}


def _window_table(windows, like):
    """[nwin][4] device table of (alpha, beta, lo, hi) per window (None: the identity), built once per (device, windows)."""
    key = (like.device, windows)
    t = _window_tables.get(key)
    if t is None:
        t = torch.tensor([v for w in windows for v in (w if w is not None else _IDENTITY_WINDOW)], dtype=torch.float32)
        t = t.to(like.device)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()    # later calls may read it from another stream
        _window_tables[key] = t
    return t


class _WindowStack(torch.autograd.Function):
    """Outputs: one re-windowed copy of x per window, all from one launch; backward: one launch for all of them."""

    @staticmethod
    def forward(ctx, x, windows):
        _dev(x)
        x = nhwc(x)
        win = _window_table(windows, x)
        outs = [torch.empty_like(x, memory_format=CL) for _ in windows]
        o = outs + [None] * (3 - len(outs))
        _L().vqw_window_stack_fwd(x, win, o[0], o[1], o[2], len(windows), x.numel())
        ctx.set_materialize_grads(False)       # an unused window's gradient arrives as None (the kernel takes a null pointer)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, win)
            ctx.nwin = len(windows)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        x, win = ctx.saved_tensors
        g = [None if t is None else nhwc(t) for t in gs] + [None] * (3 - len(gs))
        gx = torch.empty_like(x, memory_format=CL)
        _L().vqw_window_stack_bwd(x, win, g[0], g[1], g[2], gx, ctx.nwin, x.numel())
        return gx, None


def window_stack(x, windows):
    """One re-windowed copy of x per window, w(x) = clamp(alpha * x + beta, lo, hi): `windows` is a tuple of one to three
    windows, each None (the identity) or the (alpha, beta, lo, hi) of `window_map`.  All copies come from one read of x in one
    kernel, the identity's too: every output is a fresh channels-last tensor, and x receives ONE gradient, the sum over the
    windows that have one (slope inside (lo, hi), zero elsewhere), from one kernel.  Without x.requires_grad no tape is kept."""
    windows = tuple(None if w is None else tuple(float(v) for v in w) for w in windows)
    if not 1 <= len(windows) <= 3 or any(w is not None and len(w) != 4 for w in windows):
        raise RuntimeError("window_stack: one to three windows, each None or the (alpha, beta, lo, hi) of window_map")
    return _WindowStack.apply(x, windows)


def _pc_ohwi(w):
    """The layer's weight as OHWI (channels_last) fp32, kept while the weight is unchanged."""
    return _cached(w, "pc_ohwi", lambda: nhwc(w.detach().float()).clone())


def _pc_stem(w1, C):
    """The stem weight the kernels read: w1 summed over its 3 input channels for a 1-channel input (expand() feeds the
    same value to all three), w1 itself for a 3-channel one."""
    if C == 3:
        return _pc_ohwi(w1)
    return _cached(w1, "pc_stem1", lambda: nhwc(w1.detach().float().sum(dim=1, keepdim=True)).clone())


def _pc_conv(L, x, w, b, Cin, Cout, N, H, W, relu):
    """3x3 'same' convolution of the VGG slice: Winograd form where served (no max-pool follows these layers), else direct."""
    y = empty_nhwc(N, Cout, H, W, x)
    if L.vqw_conv3x3_wino_supported(Cin, Cout, N, H, W):
        u = _cached(w, "pc_wino", lambda: _wino_weights(L, _pc_ohwi(w), Cin, Cout))
        L.vqw_conv3x3_wino_fwd(x, u, b, y, N, H, W, Cin, Cout, int(relu))
    else:
        L.vqw_conv2d_fwd(x, Cin, 0, None, 0, _pc_ohwi(w), b, y, N, H, W, Cout, 3, 1, int(relu))
    return y


def _pc_dgrad(L, gy, w, mask, Cin, Cout, N, H, W):
    """Input gradient of a 3x3 layer (Cin -> Cout) from gy, zeroed where mask <= 0 (the ReLU in front of the layer; mask =
    that ReLU's output) when a mask is given."""
    gx = empty_nhwc(N, Cin, H, W, gy)
    masked_wino = mask is not None and L.vqw_conv3x3_wino_masked_supported(Cout, Cin, N, H, W)
    if masked_wino or (mask is None and L.vqw_conv3x3_wino_supported(Cout, Cin, N, H, W)):
        u = _cached(w, "pc_wino_dgrad", lambda: _wino_weights_dgrad(L, _pc_ohwi(w), Cout, Cin))
        if masked_wino:
            L.vqw_conv3x3_wino_fwd_masked(gy, u, mask, gx, N, H, W, Cout, Cin)
        else:
            L.vqw_conv3x3_wino_fwd(gy, u, None, gx, N, H, W, Cout, Cin, 0)
        return gx

    def _pack():
        buf = torch.empty(Cin * 9 * Cout, dtype=torch.float32, device=gy.device)
        L.vqw_pack_dgrad_weights(_pc_ohwi(w), buf, Cout, Cin, 3)
        return buf
    wt = _cached(w, "pc_dgrad", _pack)
    L.vqw_conv2d_fwd(gy, Cout, 0, None, 0, wt, None, gx, N, H, W, Cin, 3, 1, 0)
    if mask is not None:
        L.vqw_relu_bwd(mask, gx, gx, gx.numel())
    return gx


class _PerceptualLoss(torch.autograd.Function):
    """Outputs: one 0-dim loss per window.  The batch of every launch is 2M = 2 * nwin * N images, the sr half first."""

    @staticmethod
    def forward(ctx, sr, hr, windows, w1, b1, w2, b2, w3, b3, w4, b4):
        _dev(sr, hr)
        sr, hr = nhwc(sr), nhwc(hr)
        if sr.shape != hr.shape:
            raise RuntimeError("perceptual_loss: shape mismatch %s vs %s" % (tuple(sr.shape), tuple(hr.shape)))
        N, C, H, W = sr.shape
        L = _L()
        if C not in (1, 3) or not L.vqw_percep_supported(N, C, H, W):
            raise RuntimeError("perceptual_loss: input (N, C, H, W) = %s is not served: C must be 1 or 3 (the reference "
                               "expands to 3 channels) and H, W at least 2" % (tuple(sr.shape),))
        nwin = len(windows)
        M, h, w = nwin * N, H // 2, W // 2
        win = _window_table(windows, sr) if any(x is not None for x in windows) or nwin > 1 else None
        ws1 = _pc_stem(w1, C)
        b1, b2, b3 = _flat(b1.detach()), _flat(b2.detach()), _flat(b3.detach())
        a1 = empty_nhwc(2 * M, 64, H, W, sr)                       # conv1_1 + ReLU
        L.vqw_percep_stem_fwd(sr, hr, ws1, b1, win, a1, N, nwin, C, H, W)
        r12 = empty_nhwc(2 * M, 64, H, W, sr)                      # conv1_2 + ReLU: direct form (ties of the pool behind it)
        L.vqw_conv2d_fwd(a1, 64, 0, None, 0, _pc_ohwi(w2), b2, r12, 2 * M, H, W, 64, 3, 1, 1)
        p1 = empty_nhwc(2 * M, 64, h, w, sr)
        L.vqw_maxpool2_fwd(r12, p1, 2 * M, H, W, 64)
        a2 = _pc_conv(L, p1, w3, b3, 64, 128, 2 * M, h, w, True)  # conv2_1 + ReLU
        d = empty_nhwc(M, 128, h, w, sr)
        L.vqw_percep_diff(a2, d, d.numel())
        y = _pc_conv(L, d, w4, None, 128, 128, M, h, w, False)    # conv2_2 before its ReLU: vgg(sr) - vgg(hr)
        loss = torch.empty(nwin, dtype=torch.float32, device=sr.device)
        lws = _ws(L.vqw_percep_loss_ws_bytes(nwin), sr)
        L.vqw_percep_loss_fwd(y, loss, lws, lws.numel(), nwin, N * 128 * h * w)
        ctx.save_for_backward(sr, a1[:M], r12[:M], p1[:M], a2[:M], y)
        ctx.weights = (w1, w2, w3, w4)
        ctx.win = win
        ctx.shape = (N, nwin, C, H, W)
        return loss[0] if nwin == 1 else tuple(loss.unbind())

    @staticmethod
    def backward(ctx, *gl):
        none = (None,) * 11
        if not ctx.needs_input_grad[0]:
            return none
        sr, a1, r12, p1, a2, y = ctx.saved_tensors
        w1, w2, w3, w4 = ctx.weights
        N, nwin, C, H, W = ctx.shape
        M, h, w = nwin * N, H // 2, W // 2
        L = _L()
        dz2 = _pc_dgrad(L, y, w4, a2, 128, 128, M, h, w)           # conv2_2^T, ReLU of conv2_1
        dp1 = _pc_dgrad(L, dz2, w3, None, 64, 128, M, h, w)        # conv2_1^T
        L.vqw_relu_bwd(p1, dp1, dp1, dp1.numel())   # ReLU of conv1_2, pooled
        dr12 = empty_nhwc(M, 64, H, W, sr)
        L.vqw_maxpool2_bwd(r12, dp1, None, dr12, M, H, W, 64)
        dz1 = _pc_dgrad(L, dr12, w2, a1, 64, 64, M, H, W)          # conv1_2^T, ReLU of conv1_1
        gs = [g.contiguous() for g in gl]
        gs += [None] * (3 - len(gs))
        gsr = torch.empty_like(sr, memory_format=CL)
        L.vqw_percep_stem_bwd(sr, _pc_stem(w1, C), ctx.win, gs[0], gs[1], gs[2],
                              dz1, gsr, N, nwin, C, H, W, N * 128 * h * w)
        return (gsr,) + none[1:]


def perceptual_loss(sr, hr, w1, b1, w2, b2, w3, b3, w4, b4, window=None, windows=None):
    """F.mse_loss(vgg(sr), vgg(hr)) of the reference's VGGLoss(conv_index='22'): vgg = vgg19.features[:8] (conv1_1, ReLU,
    conv1_2, ReLU, MaxPool2d(2), conv2_1, ReLU, conv2_2 - the output is taken before the last ReLU) on the inputs expanded
    to 3 channels.  w1..w4 / b1..b4: the four convolutions' weights (OIHW, [64,3,3,3] ... [128,128,3,3]) and biases.
    The gradient flows to sr only; hr and the weights get none.
    window = (alpha, beta, lo, hi) of `window_map`: both images are re-windowed inside the kernels first.  windows = a tuple
    of such windows (None: the identity), all evaluated in one batch: returns one loss per window."""
    single = windows is None
    if single:
        windows = (window,)
    elif window is not None:
        raise RuntimeError("perceptual_loss: pass window or windows, not both")
    windows = tuple(None if x is None else tuple(float(v) for v in x) for x in windows)
    if not 1 <= len(windows) <= 3 or any(x is not None and len(x) != 4 for x in windows):
        raise RuntimeError("perceptual_loss: one to three windows, each the (alpha, beta, lo, hi) of window_map")
    out = _PerceptualLoss.apply(sr, hr.detach(), windows, w1, b1, w2, b2, w3, b3, w4, b4)
    return out if single or isinstance(out, tuple) else (out,)


# ----------------------------------------------------------------------------------------------
# LPIPS perceptual loss (functions/lpips_loss.py: lpips.LPIPS(net='alex') v0.1, csrc/lpips.hip)
# ----------------------------------------------------------------------------------------------
LPIPS_CHANNELS = (64, 192, 384, 256, 256)      # the five taps


def lpips_map_sizes(H, W):
    """((h, w) of taps 0..4) for an H x W input: conv 11/4 pad 2, pool 3/2, (5x5 same), pool 3/2, (3x3 same) x 3."""
    s0 = ((H - 7) // 4 + 1, (W - 7) // 4 + 1)
    s1 = ((s0[0] - 3) // 2 + 1, (s0[1] - 3) // 2 + 1)
    s2 = ((s1[0] - 3) // 2 + 1, (s1[1] - 3) // 2 + 1)
    return (s0, s1, s2, s2, s2)


def _lp_stem(w1, shift, scale, C):
    """(wp, cint, sc) of vqw_lpips_stem_fwd for a C-channel input, built in double from the [64,3,11,11] weight and the
    scaling layer's buffers and kept while they are unchanged."""
    def _build():
        w = w1.detach().double()
        sh, sc = shift.detach().double().reshape(3), scale.detach().double().reshape(3)
        if C == 3:
            wp = w.permute(1, 2, 3, 0).reshape(3, 121, 64).float().contiguous()
            return wp, None, torch.cat([sh, sc]).float().contiguous()
        wa = (w / sc.view(1, 3, 1, 1)).sum(1)
        wb = -(w * (sh / sc).view(1, 3, 1, 1)).sum(1)
        wp = torch.stack([wa, wb]).permute(0, 2, 3, 1).reshape(2, 121, 64).float().contiguous()
        rows = wp[1].cpu()
        cint = torch.zeros(64, dtype=torch.float32)
        for t in range(121):                      # the kernel's own order: one fp32 add per tap
            cint = cint + rows[t]
        return wp, cint.to(w1.device), None
    return _cached(w1, "lp_stem%d" % C, _build, deps=(shift, scale))


def _lp_lin(lw):
    return _cached(lw, "lp_lin", lambda: lw.detach().float().reshape(-1).contiguous())


def _lp_dgrad5(L, w, Cin, Cout):
    def _pack():
        buf = torch.empty(Cin * 25 * Cout, dtype=torch.float32, device=w.device)
        L.vqw_pack_dgrad_weights(_pc_ohwi(w), buf, Cout, Cin, 5)
        return buf
    return _cached(w, "lp_dgrad5", _pack)


class _LpipsLoss(torch.autograd.Function):
    """Outputs: one 0-dim loss per window.  The batch of every launch is 2M = 2 * nwin * N images, the sr half first."""

    @staticmethod
    def forward(ctx, sr, hr, windows, *params):
        w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = params[:10]
        lins, shift, scale = params[10:15], params[15], params[16]
        _dev(sr, hr)
        sr, hr = nhwc(sr), nhwc(hr)
        if sr.shape != hr.shape:
            raise RuntimeError("lpips_loss: shape mismatch %s vs %s" % (tuple(sr.shape), tuple(hr.shape)))
        N, C, H, W = sr.shape
        L = _L()
        if C not in (1, 3) or not L.vqw_lpips_supported(N, C, H, W):
            raise RuntimeError("lpips_loss: input (N, C, H, W) = %s is not served: C must be 1 or 3 (the reference expands "
                               "to 3 channels) and H, W at least 31 (the second max-pool needs a 3-wide map)"
                               % (tuple(sr.shape),))
        nwin = len(windows)
        M = nwin * N
        sizes = lpips_map_sizes(H, W)
        win = _window_table(windows, sr) if any(x is not None for x in windows) or nwin > 1 else None
        wp, cint, sc = _lp_stem(w1, shift, scale, C)
        (h0, w0), (h1, w1_), (h2, w2_) = sizes[0], sizes[1], sizes[2]
        if not L.vqw_lpips_conv5_supported(64, 192, 2 * M, h1, w1_):
            raise RuntimeError("lpips_loss: batch of %d images of %d x %d is too large for one launch" % (2 * M, H, W))
        f0 = empty_nhwc(2 * M, 64, h0, w0, sr)
        L.vqw_lpips_stem_fwd(sr, hr, wp, cint, sc, _flat(b1.detach()), win, f0, N, nwin, C, H, W)
        p0 = empty_nhwc(2 * M, 64, h1, w1_, sr)
        L.vqw_lpips_pool_fwd(f0, p0, 2 * M, h0, w0, 64)
        f1 = empty_nhwc(2 * M, 192, h1, w1_, sr)
        L.vqw_lpips_conv5_fwd(p0, _pc_ohwi(w2), _flat(b2.detach()), f1, 2 * M, h1, w1_, 64, 192, 1)
        p1 = empty_nhwc(2 * M, 192, h2, w2_, sr)
        L.vqw_lpips_pool_fwd(f1, p1, 2 * M, h1, w1_, 192)
        f2 = _pc_conv(L, p1, w3, _flat(b3.detach()), 192, 384, 2 * M, h2, w2_, True)
        f3 = _pc_conv(L, f2, w4, _flat(b4.detach()), 384, 256, 2 * M, h2, w2_, True)
        f4 = _pc_conv(L, f3, w5, _flat(b5.detach()), 256, 256, 2 * M, h2, w2_, True)
        feats = (f0, f1, f2, f3, f4)
        ws = _ws(L.vqw_lpips_ws_bytes(N, nwin), sr)
        for t, f in enumerate(feats):
            L.vqw_lpips_dist_fwd(f, _lp_lin(lins[t]), ws, ws.numel(), t, N, nwin, sizes[t][0] * sizes[t][1], LPIPS_CHANNELS[t])
        loss = torch.empty(nwin, dtype=torch.float32, device=sr.device)
        L.vqw_lpips_loss_fold(ws, ws.numel(), loss, N, nwin, *[h * w for h, w in sizes])
        ctx.save_for_backward(sr, *feats)
        ctx.weights = (w1, w2, w3, w4, w5, lins, shift, scale)
        ctx.win = win
        ctx.shape = (N, nwin, C, H, W)
        return loss[0] if nwin == 1 else tuple(loss.unbind())

    @staticmethod
    def backward(ctx, *gl):
        N, nwin, C, H, W = ctx.shape
        none = (None,) * 20
        if not ctx.needs_input_grad[0]:
            return none
        sr, f0, f1, f2, f3, f4 = ctx.saved_tensors
        w1, w2, w3, w4, w5, lins, shift, scale = ctx.weights
        M = nwin * N
        sizes = lpips_map_sizes(H, W)
        (h0, w0), (h1, w1_), (h2, w2_) = sizes[0], sizes[1], sizes[2]
        hw2 = h2 * w2_
        L = _L()
        # each tap: its own distance gradient + the gradient from the deeper tap, masked by its ReLU, in one launch
        dz4 = empty_nhwc(M, 256, h2, w2_, sr)
        L.vqw_lpips_dist_bwd(f4, _lp_lin(lins[4]), None, dz4, N, nwin, hw2, 256)
        g3 = _pc_dgrad(L, dz4, w5, None, 256, 256, M, h2, w2_)
        L.vqw_lpips_dist_bwd(f3, _lp_lin(lins[3]), g3, g3, N, nwin, hw2, 256)
        g2 = _pc_dgrad(L, g3, w4, None, 384, 256, M, h2, w2_)
        L.vqw_lpips_dist_bwd(f2, _lp_lin(lins[2]), g2, g2, N, nwin, hw2, 384)
        gp1 = _pc_dgrad(L, g2, w3, None, 192, 384, M, h2, w2_)
        g1 = empty_nhwc(M, 192, h1, w1_, sr)
        L.vqw_lpips_pool_bwd(f1, gp1, g1, M, h1, w1_, 192)
        L.vqw_lpips_dist_bwd(f1, _lp_lin(lins[1]), g1, g1, N, nwin, h1 * w1_, 192)
        gp0 = empty_nhwc(M, 64, h1, w1_, sr)
        L.vqw_lpips_conv5_fwd(g1, _lp_dgrad5(L, w2, 64, 192), None, gp0, M, h1, w1_, 192, 64, 0)
        g0 = empty_nhwc(M, 64, h0, w0, sr)
        L.vqw_lpips_pool_bwd(f0, gp0, g0, M, h0, w0, 64)
        L.vqw_lpips_dist_bwd(f0, _lp_lin(lins[0]), g0, g0, N, nwin, h0 * w0, 64)
        gs = [g.contiguous() for g in gl]
        gs += [None] * (3 - len(gs))
        wp, _, sc = _lp_stem(w1, shift, scale, C)
        gsr = torch.empty_like(sr, memory_format=CL)
        L.vqw_lpips_stem_bwd(sr, wp, sc, ctx.win, gs[0], gs[1], gs[2], g0, gsr, N, nwin, C, H, W)
        return (gsr,) + none[1:]


def lpips_loss(sr, hr, params, window=None, windows=None):
    """lpips.LPIPS(net='alex') v0.1 (linear layers on, spatial=False, eval mode, normalize=False) of sr against hr, mean over
    the batch: the reference's LPIPSLoss.  params: (w1, b1, ..., w5, b5, lin0, ..., lin4, shift, scale) - the five
    convolutions of alexnet.features (OIHW: [64,3,11,11], [192,64,5,5], [384,192,3,3], [256,384,3,3], [256,256,3,3]) with
    their biases, the five 1x1 lin weights ([1,C,1,1], no bias) and the scaling layer's shift / scale ([1,3,1,1]).  Inputs are
    (N, 1 or 3, H, W) in [-1, 1] with H, W >= 31; a 1-channel input stands for its expand() to 3.  The gradient flows to sr
    only; hr and the parameters get none.  At a pixel whose tap features are all zero the normalisation contributes a zero
    gradient (autograd through sqrt gives NaN there, which the ReLU's backward then discards).  window / windows: as in `perceptual_loss`."""
    single = windows is None
    if single:
        windows = (window,)
    elif window is not None:
        raise RuntimeError("lpips_loss: pass window or windows, not both")
    windows = tuple(None if x is None else tuple(float(v) for v in x) for x in windows)
    if not 1 <= len(windows) <= 3 or any(x is not None and len(x) != 4 for x in windows):
        raise RuntimeError("lpips_loss: one to three windows, each the (alpha, beta, lo, hi) of window_map")
    params = tuple(params)
    if len(params) != 17:
        raise RuntimeError("lpips_loss: params must be the 17 tensors (w1, b1, ..., w5, b5, lin0 .. lin4, shift, scale)")
    out = _LpipsLoss.apply(sr, hr.detach(), windows, *params)
    return out if single or isinstance(out, tuple) else (out,)


METRIC_SLOTS = ("mse", "ssim", "psnr", "ssim_range", "psnr_range", "sse", "target_min", "target_max", "entropy", "bad_ids",
                "n_ids")
_MT_OUT = 16


def _dense_storage(t):
    """1-D view of a tensor's elements in storage order, without a copy when the tensor is a permutation of a dense
    layout (the encoder's ids are a transposed view, unet_encoder.py:86); otherwise a contiguous copy.  Counting over
    it counts the same multiset of values."""
    if t.is_contiguous():
        return t.reshape(-1)
    dims = sorted((s, n) for s, n in zip(t.stride(), t.shape) if n != 1)
    expect = 1
    for s, n in dims:
        if s != expect:
            return t.contiguous().reshape(-1)
        expect *= n
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


def _image_pair(pred, target, name):
    pred, target = pred.detach(), target.detach()
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise RuntimeError("%s: pred and target must be fp32 (got %s, %s)" % (name, pred.dtype, target.dtype))
    if pred.shape != target.shape:
        raise RuntimeError("%s: shape mismatch %s vs %s" % (name, tuple(pred.shape), tuple(target.shape)))
    return pred, target


def _ids_arg(ids, dict_size, name):
    if dict_size is None:
        raise RuntimeError("%s: ids need dict_size" % name)
    _dev(ids)
    ids = _dense_storage(ids.detach())
    if ids.dtype != torch.int64:
        raise RuntimeError("%s: ids must be int64 (got %s)" % (name, ids.dtype))
    if ids.numel() == 0:
        raise RuntimeError("%s: no ids" % name)
    return ids


def _metrics_launch(pred, target, ids, dict_size, data_range, kernel_size, sigma, k1, k2, counts=None):
    """-> out (16,) float64 device tensor of METRIC_SLOTS; four launches at most, no synchronisation."""
    like = pred if pred is not None else ids
    if pred is not None:
        N, C, H, W = pred.shape
    else:
        N = C = H = W = 0
    K = int(dict_size) if ids is not None else 0
    out = torch.empty(_MT_OUT, dtype=torch.float64, device=like.device)
    L = _L()
    ws = _ws(L.vqw_recon_metrics_ws_bytes(N, C, H, W, K), like)
    dr = float(data_range) if data_range is not None else 0.0
    L.vqw_recon_metrics(pred, target, ids, out, counts, ws, ws.numel(), N, C, H, W, ids.numel() if ids is not None else 0,
                        K, int(kernel_size), float(sigma), float(k1), float(k2), dr)
    return out


def _check_ids(host, name):
    if host[METRIC_SLOTS.index("bad_ids")] > 0:
        raise ValueError("%s: %d ids outside [0, dict_size]" % (name, int(host[METRIC_SLOTS.index("bad_ids")])))


def image_metrics_raw(pred, target, data_range=None, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """Streaming statistics of any two equal-shape fp32 tensors (kernel_size=0: no SSIM pass, any shape) or the full
    (N, C, H, W) set with SSIM -> the (16,) float64 device tensor of METRIC_SLOTS.  Used by the torchmetrics drop-ins."""
    pred, target = _image_pair(pred, target, "image_metrics")
    if kernel_size:
        kernel_size, sigma = _recon_metrics_check(pred, kernel_size, sigma)
    if pred.numel() == 0:
        raise RuntimeError("image_metrics: empty input")
    _dev(pred, target)
    pred, target = pred.contiguous(), target.contiguous()     # no copy for C = 1 (NCHW and NHWC coincide)
    if not kernel_size:
        pred, target = pred.reshape(1, 1, 1, -1), target.reshape(1, 1, 1, -1)
    return _metrics_launch(pred, target, None, None, data_range, kernel_size, sigma, k1, k2)


def _recon_metrics_check(pred, kernel_size, sigma):
    if isinstance(kernel_size, (tuple, list)) or isinstance(sigma, (tuple, list)):
        ks, sg = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size,) * 2, \
            tuple(sigma) if isinstance(sigma, (tuple, list)) else (sigma,) * 2
        if len(ks) != 2 or len(sg) != 2 or ks[0] != ks[1] or sg[0] != sg[1]:
            raise NotImplementedError("recon_metrics: only square SSIM windows are built (kernel_size=%r, sigma=%r)"
                                      % (kernel_size, sigma))
        kernel_size, sigma = ks[0], sg[0]
    kernel_size = int(kernel_size)
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError("recon_metrics: kernel_size must be odd and positive (got %d)" % kernel_size)
    if not float(sigma) > 0:
        raise ValueError("recon_metrics: sigma must be > 0 (got %r)" % (sigma,))
    if pred.dim() != 4:
        raise RuntimeError("recon_metrics: expected (N, C, H, W) inputs, got shape %s" % (tuple(pred.shape),))
    H, W = pred.shape[-2:]
    if H < kernel_size or W < kernel_size:
        raise ValueError("recon_metrics: H=%d and W=%d must be at least kernel_size=%d" % (H, W, kernel_size))
    return kernel_size, float(sigma)


def _recon_metrics_out(pred, target, ids, dict_size, data_range, kernel_size, sigma, k1, k2):
    pred, target = _image_pair(pred, target, "recon_metrics")
    kernel_size, sigma = _recon_metrics_check(pred, kernel_size, sigma)
    if data_range is not None and not float(data_range) > 0:
        raise ValueError("recon_metrics: data_range must be > 0 (got %r)" % (data_range,))
    _dev(pred, target)
    pred, target = pred.contiguous(), target.contiguous()     # no copy for C = 1 (NCHW and NHWC coincide)
    if ids is not None:
        ids = _ids_arg(ids, dict_size, "recon_metrics")
    return _metrics_launch(pred, target, ids, dict_size, data_range, kernel_size, sigma, k1, k2)


def recon_metrics(pred, target, ids=None, dict_size=None, data_range=None, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03):
    """The per-batch metrics of the reference's test step (single_window_trainer.py:781-827) as torchmetrics 0.6.2 and
    scipy compute them -> {'mse', 'ssim', 'psnr'[, 'entropy']} as 0-d float64 device tensors (not differentiable).

    mse: mean (pred - target)^2.  ssim: mean over the valid kernel_size^2 Gaussian windows of every (n, c) plane with
    C1 = (k1 R)^2, C2 = (k2 R)^2, R = max(range pred, range target) over the batch.  psnr: 10 log10(R'^2 / mse) with the
    package's zero-seeded R' = max(max target, 0) - min(min target, 0).  A given data_range replaces R and R'.
    entropy (with ids and dict_size K): base-2 entropy of the counts of ids 1..K (id 0 = no code); ids outside [0, K]
    raise, which reads the results to the host once.  Without ids nothing synchronises."""
    out = _recon_metrics_out(pred, target, ids, dict_size, data_range, kernel_size, sigma, k1, k2)
    if ids is not None:
        _check_ids(out.cpu().tolist(), "recon_metrics")
    res = dict(mse=out[0], ssim=out[1], psnr=out[2])
    if ids is not None:
        res["entropy"] = out[METRIC_SLOTS.index("entropy")]
    return res


def recon_metrics_values(pred, target, ids=None, dict_size=None, data_range=None, kernel_size=11, sigma=1.5, k1=0.01,
                         k2=0.03):
    """recon_metrics as Python floats, with one device-to-host read of the results."""
    out = _recon_metrics_out(pred, target, ids, dict_size, data_range, kernel_size, sigma, k1, k2)
    host = out.cpu().tolist()
    if ids is not None:
        _check_ids(host, "recon_metrics")
    keys = ("mse", "ssim", "psnr") + (("entropy",) if ids is not None else ())
    return {k: host[METRIC_SLOTS.index(k)] for k in keys}


def code_entropy(ids, dict_size):
    """-> (entropy, counts): scipy.stats.entropy(bincount(ids, minlength=K+1)[1:], base=2) as a 0-d float64 device
    tensor (nan when no id is in 1..K) and the (K + 1,) int64 device counts of ids 0..K.  ids may be any dense view (no
    copy); ids outside [0, K] raise (one host read)."""
    ids = _ids_arg(ids, dict_size, "code_entropy")
    K = int(dict_size)
    out = torch.empty(_MT_OUT, dtype=torch.float64, device=ids.device)
    counts = torch.empty(K + 1, dtype=torch.int64, device=ids.device)
    L = _L()
    ws = _ws(L.vqw_recon_metrics_ws_bytes(0, 0, 0, 0, K), ids)
    L.vqw_code_entropy(ids, out, counts, ws, ws.numel(), ids.numel(), K)
    _check_ids(out.cpu().tolist(), "code_entropy")
    return out[METRIC_SLOTS.index("entropy")], counts


class _WeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *terms):
        dev = terms[0].device
        _dev(*terms)
        terms = [t.reshape(()).contiguous() for t in terms]
        out = torch.empty((), dtype=torch.float32, device=dev)
        if len(terms) <= 16:
            # pointers and weights travel as kernel arguments: no device-side table, no host-to-device copy (a blocking
            # copy synchronises the stream — the host would wait for the whole forward pass before it can enqueue the
            # backward pass —, a pinned staging buffer per call makes the host allocator wait for the device now and then)
            tp = (ctypes.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
            tw = (ctypes.c_float * len(terms))(*[float(x) for x in weights])
            _lib.check(_lib.load().vqw_weighted_sum_host(tp, tw, len(terms), _raw(out), _raw_stream()), "vqw_weighted_sum_host")
        else:
            ptrs = torch.tensor([t.data_ptr() for t in terms], dtype=torch.int64).to(dev)
            w = torch.tensor(list(weights), dtype=torch.float32).to(dev)
            _L().vqw_weighted_sum(ptrs, w, len(terms), out)
        ctx.weights = list(weights)
        ctx.keep = terms
        return out

    @staticmethod
    def backward(ctx, g):
        gs = []
        for wgt, need in zip(ctx.weights, ctx.needs_input_grad[1:]):
            if not need:
                gs.append(None)
                continue
            o = torch.empty((), dtype=torch.float32, device=g.device)
            gc = g.contiguous()
            _L().vqw_affine(gc, o, float(wgt), 0.0, 1)
            gs.append(o)
        return (None, *gs)


def weighted_sum(terms, weights):
    """sum_i weights[i] * terms[i] for 0-dim device tensors (single_window_trainer.py:131-137)."""
    return _WeightedSum.apply(tuple(float(w) for w in weights), *terms)


# ----------------------------------------------------------------------------------------------
# vector quantisation
# ----------------------------------------------------------------------------------------------
class _VQ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, embed, cluster_size, embed_avg, training, momentum, eps, dist_mode, id_base, torch_ema_weight):
        _dev(x, embed, cluster_size, embed_avg)
        x = nhwc(x)
        N, D, H, W = x.shape
        K = embed.shape[0]
        if embed.shape[1] != D:
            raise RuntimeError("VQ: emb_dim %d does not match input channels %d" % (embed.shape[1], D))
        L = _L()
        npix = N * H * W
        ids = torch.empty((N, H, W), dtype=torch.int64, device=x.device)
        q = torch.empty_like(x, memory_format=CL)
        commit = torch.empty((), dtype=torch.float32, device=x.device)
        stats = torch.empty(K + D * K, dtype=torch.float64, device=x.device) if training else None
        ws = _ws(L.vqw_vq_ws_bytes(npix, D, K), x)
        if not (embed.is_contiguous() and cluster_size.is_contiguous() and embed_avg.is_contiguous()):
            raise RuntimeError("VQ buffers must be contiguous")
        cur = _order_begin(embed)        # the codebook read AND its EMA update stay in program order across streams
        L.vqw_vq_fwd(x, embed, ids, int(id_base), q, commit, stats, ws, ws.numel(), npix, D, K)
        if training:
            scale = 1.0
            if _dist_on() and dist_mode != "local":
                if dist_mode == "global":
                    _all_reduce(stats)                  # counts and sums over the global batch
                elif dist_mode == "reference":
                    # vq_module.py:187-193: embed_sum rank-averaged, counts local (C3 quirk; C2's dead
                    # N x K all-reduce is never reproduced)
                    _all_reduce(stats[K:])
                    scale = 1.0 / dist.get_world_size()
                else:
                    raise RuntimeError("unknown VQ dist_mode %r" % dist_mode)
            if torch_ema_weight:         # the double 1 - momentum, rounded once by the call: torch's add_(update, alpha=1 - momentum)
                L.vqw_vq_ema_update_w(stats, embed, cluster_size, embed_avg, momentum, 1.0 - momentum, eps, scale, D, K)
            else:
                L.vqw_vq_ema_update(stats, embed, cluster_size, embed_avg, momentum, eps, scale, D, K)
        _order_end(embed, cur)
        ctx.save_for_backward(x, q)
        ctx.mark_non_differentiable(ids)
        ctx.set_materialize_grads(False)       # no zero-filled gradient for the ids; an unused q / commit arrives as None
        return q, commit, ids

    @staticmethod
    def backward(ctx, gq, gcommit, _gids):
        if gq is None and gcommit is None:
            return (None,) * 10
        x, q = ctx.saved_tensors
        gq = nhwc(gq) if gq is not None else None
        gc = gcommit.contiguous() if gcommit is not None else None
        gx = torch.empty_like(x, memory_format=CL)
        _L().vqw_vq_bwd(x, q, gq, gc, gx, x.numel())
        return gx, None, None, None, None, None, None, None, None, None


def vq_quantize(x, embed, cluster_size, embed_avg, training, momentum, eps, dist_mode="global", id_base=0, torch_ema_weight=False):
    """-> (quantized with straight-through gradient, commit loss, ids (N,H,W) int64 = code + id_base, per pixel).
    torch_ema_weight: the EMA weighs the new statistics with the double 1 - momentum rounded once, as torch does, instead of
    1.f - momentum formed in float32 (the default, which the U-Net models' recorded steps were taken with)."""
    return _VQ.apply(x, embed, cluster_size, embed_avg, bool(training), float(momentum), float(eps), dist_mode, int(id_base),
                     bool(torch_ema_weight))


def kmeans_codebook(features, dict_size, seed=0, tol=1e-4, max_iter=100, return_ids=False):
    """Lloyd's k-means over pixel features (P, D) -> centres (K, D): what kmeans_pytorch.kmeans (the reference's codebook
    initialisation, unet_encoder.py:77-82) computes.  Own semantics (the dependency is absent, parity unpinned): centres
    start from K distinct random rows (seeded), an iteration = nearest-centre assignment + per-centre mean (the VQ search /
    statistics kernels and vqw_kmeans_update), empty clusters keep their centre, stop when (sum_k |delta_k|)^2 < tol as
    kmeans_pytorch does, or after max_iter.  Returns (centres, list of (mean squared distance per row, shift, empty codes)
    per iteration) and, with return_ids, the assignment of the last search (oracle/kmeans_ref.py restates this on the CPU)."""
    _dev(features)
    P, D = features.shape
    if P < dict_size:
        raise RuntimeError("k-means needs at least dict_size = %d feature rows, got %d" % (dict_size, P))
    L = _L()
    x = features.detach().contiguous().float()
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    centres = x[torch.randperm(P, generator=g)[:dict_size].to(x.device)].clone()
    ids = torch.empty(P, dtype=torch.int64, device=x.device)
    q = torch.empty_like(x)
    commit = torch.empty((), dtype=torch.float32, device=x.device)
    stats = torch.empty(dict_size + D * dict_size, dtype=torch.float64, device=x.device)
    shift = torch.empty(2, dtype=torch.float64, device=x.device)
    ws = _ws(L.vqw_vq_ws_bytes(P, D, dict_size), x)
    ws2 = _ws(16 * dict_size, x)
    history = []
    for _ in range(int(max_iter)):
        L.vqw_vq_fwd(x, centres, ids, 0, q, commit, stats, ws, ws.numel(), P, D, dict_size)
        L.vqw_kmeans_update(stats, centres, shift, ws2, ws2.numel(), D, dict_size)
        sh = shift.tolist()                      # one host sync per iteration of a one-off initialisation
        history.append((float(commit) * D, sh[0], int(sh[1])))       # commit = mean squared distance per element -> per row
        if sh[0] ** 2 < tol:
            break
    return (centres, history, ids) if return_ids else (centres, history)


def vq_lookup(ids, embed, mask=None, scale=None):
    """embed[ids] as (N,D,H,W) NHWC; optional mask (uint8 (N,H,W)) and device scalar scale."""
    _dev(ids, embed)
    if ids.dtype != torch.int64:
        ids = ids.long()
    ids = ids.contiguous()
    N, H, W = ids.shape
    K, D = embed.shape
    out = empty_nhwc(N, D, H, W, embed)
    _L().vqw_vq_lookup(ids, embed.contiguous(), mask, scale, out, N * H * W, D, K)
    return out


def mask_scale(label_map):
    """run_recon.py:179-192: -> (mask uint8, ids0 int64, scale (1,) float32 = numel/sum(mask))."""
    _dev(label_map)
    lab = label_map.long().contiguous()
    mask = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
    ids0 = torch.empty_like(lab)
    scale = torch.empty(1, dtype=torch.float32, device=lab.device)
    _L().vqw_mask_scale(lab, mask, ids0, scale, lab.numel())
    return mask, ids0, scale


# ----------------------------------------------------------------------------------------------
# embedding loss
# ----------------------------------------------------------------------------------------------
class _CrossLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embed, labels_or_r, codebook_kd, dense):
        _dev(embed, labels_or_r, codebook_kd)
        e = nhwc(embed)
        B, D, H, W = e.shape
        K = codebook_kd.shape[0]
        cb = codebook_kd.detach().contiguous()
        L = _L()
        loss = torch.empty((), dtype=torch.float32, device=e.device)
        coef = torch.empty(B * K, dtype=torch.float32, device=e.device)
        ws = _ws(L.vqw_cross_ws_bytes(B, K, H * W), e)
        if dense:
            r = labels_or_r.contiguous()
            if tuple(r.shape) != (B, K, H, W) or r.dtype != torch.float32:
                raise RuntimeError("cross loss: r_ids must be float (B,K,H,W) = %s, got %s" % ((B, K, H, W), tuple(r.shape)))
            L.vqw_cross_loss_dense_fwd(e, r, cb, loss, coef, ws, ws.numel(), B, H * W, D, K)
        else:
            r = labels_or_r.contiguous()
            if tuple(r.shape) != (B, H, W) or r.dtype != torch.int32:
                raise RuntimeError("cross loss: labels must be int32 (B,H,W)")
            L.vqw_cross_loss_fwd(e, r, cb, loss, coef, ws, ws.numel(), B, H * W, D, K)
        ctx.save_for_backward(e, r, cb, coef)
        ctx.dense = dense
        return loss

    @staticmethod
    def backward(ctx, g):
        e, r, cb, coef = ctx.saved_tensors
        B, D, H, W = e.shape
        K = cb.shape[0]
        g = g.contiguous()
        ge = torch.empty_like(e, memory_format=CL)
        fn = _L().vqw_cross_loss_dense_bwd if ctx.dense else _L().vqw_cross_loss_bwd
        fn(e, r, cb, coef, g, ge, B, H * W, D, K)
        return ge, None, None, None


def cross_loss_labels(embed, labels, codebook_kd):
    return _CrossLoss.apply(embed, labels, codebook_kd, False)


def cross_loss_dense(embed, r, codebook_kd):
    return _CrossLoss.apply(embed, r, codebook_kd, True)


def codebook_losses(codebook_kd, margin):
    """(l_dist, l_reg) of embed_loss.py:68-88; the codebook is a buffer -> no gradient."""
    _dev(codebook_kd)
    cb = codebook_kd.detach().contiguous()
    K, D = cb.shape
    ld = torch.empty((), dtype=torch.float32, device=cb.device)
    lr = torch.empty((), dtype=torch.float32, device=cb.device)
    ws = _ws(16 * K, cb)
    _L().vqw_codebook_losses(cb, float(margin), ld, lr, ws, ws.numel(), D, K)
    return ld, lr


def onehot(labels, n_classes):
    _dev(labels)
    lab = labels.to(torch.int32).contiguous()
    B = lab.shape[0]
    hw = lab.numel() // B
    out = torch.empty((B, n_classes) + tuple(lab.shape[1:]), dtype=torch.float32, device=lab.device)
    _L().vqw_onehot(lab, out, B, hw, n_classes)
    return out


def flip_labels(ids, border=0):
    """Cross-view id map for identity / h-flip views: int32 (B,H,W), 0 inside `border`."""
    _dev(ids)
    ids = ids.long().contiguous()
    B, H, W = ids.shape
    out = torch.empty((B, H, W), dtype=torch.int32, device=ids.device)
    _L().vqw_flip_labels(ids, out, int(border), B, H, W)
    return out


# ----------------------------------------------------------------------------------------------
# two-view augmentation + id-map warps (data path: no autograd)
# ----------------------------------------------------------------------------------------------
def warp_image(x, minv):
    """x (B, C, H, W) fp32, minv (B, 3, 3) fp32 destination->source pixel matrices: bilinear resample, zero padding."""
    _dev(x, minv)
    x, minv = _flat(x), _flat(minv)
    B, C, H, W = x.shape
    if tuple(minv.shape) != (B, 3, 3):
        raise RuntimeError("warp_image: expected %s matrices, got %s" % ((B, 3, 3), tuple(minv.shape)))
    y = torch.empty_like(x)
    _L().vqw_warp_image(x, minv, y, B, C, H, W)
    return y


def warp_labels(ids, minv):
    """ids (B, H, W) int64 or int32 -> int32 map sampled with nearest neighbour through minv; 0 = out of frame."""
    _dev(ids, minv)
    if ids.dtype not in (torch.int64, torch.int32):
        raise RuntimeError("warp_labels: ids must be int64 or int32 (got %s)" % ids.dtype)
    ids = ids.contiguous()
    minv = _flat(minv)
    B, H, W = ids.shape
    if tuple(minv.shape) != (B, 3, 3):
        raise RuntimeError("warp_labels: expected %s matrices, got %s" % ((B, 3, 3), tuple(minv.shape)))
    out = torch.empty((B, H, W), dtype=torch.int32, device=ids.device)
    _L().vqw_warp_labels(ids, int(ids.dtype == torch.int64), minv, out, B, H, W)
    return out


def photometric(x, params, noise=None):
    """Per-sample brightness add, contrast multiply (clamped to [0,1]), posterize, + std * noise; params (B, 4)."""
    _dev(x, params, noise)
    x, params = _flat(x), _flat(params)
    B = x.shape[0]
    if tuple(params.shape) != (B, 4):
        raise RuntimeError("photometric: params must be (%d, 4)" % B)
    if noise is not None:
        noise = _flat(noise)
        if noise.shape != x.shape:
            raise RuntimeError("photometric: noise shape %s != %s" % (tuple(noise.shape), tuple(x.shape)))
    y = torch.empty_like(x)
    _L().vqw_photometric(x, params, noise, y, B, x.numel() // B)
    return y


def gauss_blur(x, taps, apply=None):
    """Separable Gaussian blur of (B, C, H, W) with 1-D `taps`, reflect border; apply (B,) uint8 selects samples."""
    _dev(x, taps, apply)
    x, taps = _flat(x), _flat(taps)
    B, C, H, W = x.shape
    if apply is not None:
        apply = apply.to(torch.uint8).contiguous()
        if apply.numel() != B:
            raise RuntimeError("gauss_blur: apply must have one entry per sample")
    tmp, y = torch.empty_like(x), torch.empty_like(x)
    _L().vqw_gauss_blur(x, taps, apply, tmp, y, B, C, H, W, taps.numel())
    return y


# ----------------------------------------------------------------------------------------------
# second training step: PatchGAN discriminator pieces (strided conv, BatchNorm(affine)+LeakyReLU, hinge losses)
# ----------------------------------------------------------------------------------------------
class _SConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, slope):
        _dev(x, weight, bias)
        x, w = nhwc(x), nhwc(weight)
        Cout, Cin, ks, _ = weight.shape
        N, _, H, W = x.shape
        if x.shape[1] != Cin:
            raise RuntimeError("sconv2d: input has %d channels, weight expects %d" % (x.shape[1], Cin))
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        if bias is not None:
            bias = _flat(bias)
        y = empty_nhwc(N, Cout, Ho, Wo, x)
        L = _L()
        ws = _ws(L.vqw_sconv_fwd_ws_bytes(N, H, W, Cin, Cout, ks, stride, pad), x)
        L.vqw_sconv_fwd(x, w, bias, y, ws, ws.numel(), N, H, W, Cin, Cout, ks, stride, pad, float(slope))
        ctx.save_for_backward(x, w, y if slope != 1.0 else None)
        ctx.cfg = (stride, pad, float(slope), bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        stride, pad, slope, has_bias = ctx.cfg
        L = _L()
        gy = nhwc(gy)
        Cout, Cin, ks, _ = w.shape
        N, _, H, W = x.shape
        if y is not None:
            gm = torch.empty_like(y, memory_format=CL)
            L.vqw_leaky_relu_bwd(y, gy, gm, slope, gy.numel())
            gy = gm
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x, memory_format=CL)
            ws = _ws(L.vqw_sconv_dgrad_ws_bytes(N, H, W, Cin, Cout, ks, stride, pad), gy)
            L.vqw_sconv_dgrad(gy, w, gx, ws, ws.numel(), N, H, W, Cin, Cout, ks, stride, pad)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=gy.device, memory_format=CL)
            gb = torch.empty(Cout, dtype=torch.float32, device=gy.device) if has_bias else None
            ws = _ws(L.vqw_sconv_wgrad_ws_bytes(Cin, Cout, ks, N, H, W, stride, pad), gy)
            L.vqw_sconv_wgrad(x, gy, gw, gb, ws, ws.numel(), N, H, W, Cin, Cout, ks, stride, pad, 0)
        return gx, gw, gb, None, None, None


def sconv2d(x, weight, bias=None, stride=1, padding=0, slope=1.0):
    """nn.Conv2d(k, stride in {1,2}, padding) with an optional LeakyReLU(slope) epilogue."""
    return _SConv.apply(x, weight, bias, int(stride), int(padding), float(slope))


class _ConvDown2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        _dev(x, weight, bias)
        x, w = nhwc(x), nhwc(weight)
        Cout, Cin, kh, kw = weight.shape
        N, _, H, W = x.shape
        if (kh, kw) != (3, 3) or x.shape[1] != Cin:
            raise RuntimeError("conv2d_down2: a 3x3 weight over the input's %d channels is expected, got %s" % (x.shape[1], tuple(weight.shape)))
        if bias is not None:
            bias = _flat(bias)
        y = empty_nhwc(N, Cout, H // 2, W // 2, x)
        _L().vqw_conv3s2_fwd(x, w, bias, y, N, H, W, Cin, Cout)        # refuses odd H / W and channel counts off 32
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        L = _L()
        gy = nhwc(gy)
        Cout, Cin = w.shape[:2]
        N, _, H, W = x.shape
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x, memory_format=CL)
            ws = _ws(L.vqw_conv3s2_dgrad_ws_bytes(Cin, Cout), gy)
            L.vqw_conv3s2_dgrad(gy, w, gx, ws, ws.numel(), N, H, W, Cin, Cout)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=gy.device, memory_format=CL)
            gb = torch.empty(Cout, dtype=torch.float32, device=gy.device) if ctx.has_bias else None
            ws = _ws(L.vqw_conv3s2_wgrad_ws_bytes(N, H, W, Cin, Cout), gy)
            L.vqw_conv3s2_wgrad(x, gy, gw, gb, ws, ws.numel(), N, H, W, Cin, Cout, 0)
        return gx, gw, gb


def conv2d_down2(x, weight, bias=None):
    """nn.Conv2d(C, C', 3, stride=2, padding=0) behind F.pad(x, (0, 1, 0, 1)): the VQGAN Downsample (vqgan.py:40-58).
    H and W even, both channel counts multiples of 32."""
    return _ConvDown2.apply(x, weight, bias)


class _BnLrelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, nbt, training, momentum, eps, slope, sync):
        _dev(x, gamma, beta)
        x = nhwc(x)
        gamma, beta = _flat(gamma), _flat(beta)
        N, C, H, W = x.shape
        L = _L()
        mr = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        count = float(N * H * W)
        if training:
            sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
            ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
            L.vqw_bn_partial_stats(x, sums, ws, ws.numel(), N, H * W, C)
            if sync and _dist_on():
                _all_reduce(sums)
                count *= dist.get_world_size()
            cur = _order_begin(running_mean)
            L.vqw_bn_finalize(sums, count, mr, running_mean, running_var, momentum, eps, C)
            if nbt is not None:
                _bump_counter(nbt)
            _order_end(running_mean, cur)
        else:
            L.vqw_bn_eval_stats(running_mean, running_var, mr, eps, C)
        y = torch.empty_like(x, memory_format=CL)
        L.vqw_bn_affine_fwd(x, mr, gamma, beta, y, N * H * W, C, float(slope))
        ctx.save_for_backward(x, gamma, beta, mr)
        ctx.cfg = (training, float(slope), count, sync)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mr = ctx.saved_tensors
        training, slope, count, sync = ctx.cfg
        N, C, H, W = x.shape
        L = _L()
        gy = nhwc(gy)
        sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
        ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
        L.vqw_bn_affine_bwd_reduce(x, mr, gamma, beta, gy, sums, ws, ws.numel(), N, H * W, C, slope)
        # dgamma / dbeta are this rank's sums (DDP averages parameter gradients); dx needs the global-batch sums
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        gx = torch.empty_like(x, memory_format=CL)
        if training and sync and _dist_on():
            local = sums.clone()
            _all_reduce(sums)
            L.vqw_bn_affine_bwd_apply(x, mr, gamma, beta, gy, sums, count, gx, None, None, N * H * W, C, slope, 1, 0)
            dbeta.copy_(local[0::2])
            dgamma.copy_(local[1::2])
        else:
            L.vqw_bn_affine_bwd_apply(x, mr, gamma, beta, gy, sums, count, gx, dgamma, dbeta,
                                      N * H * W, C, slope, int(training), 0)
        return gx, dgamma, dbeta, None, None, None, None, None, None, None, None


def batch_norm_lrelu(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, slope=0.2, sync=True,
                     num_batches_tracked=None):
    """nn.BatchNorm2d (affine) followed by nn.LeakyReLU(slope) (slope = 1: plain BatchNorm)."""
    return _BnLrelu.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, bool(training), float(momentum),
                          float(eps), float(slope), bool(sync))


class _ActNormLrelu(torch.autograd.Function):
    """ActNorm + LeakyReLU on the BatchNorm-affine kernels in their eval form: mean = -loc, rstd = 1, gamma = scale, beta = 0
    (`x - (-loc)`, `* 1`, `+ 0` are exact), so y = lrelu(scale * (x + loc)) bit for bit and no kernel is duplicated."""

    @staticmethod
    def forward(ctx, x, loc, scale, initialized, slope, sync):
        _dev(x, loc, scale)
        x = nhwc(x)
        N, C, H, W = x.shape
        if loc.numel() != C or scale.numel() != C:
            raise RuntimeError("act_norm_lrelu: loc / scale have %d entries, input has %d channels" % (loc.numel(), C))
        loc, scale = _flat(loc), _flat(scale)          # (1, C, 1, 1) parameters: dense, written in place when initialising
        L = _L()
        mrb = torch.empty(3 * C, dtype=torch.float32, device=x.device)       # [C][2] {-loc, 1}, then the zero beta
        if initialized is not None:                    # data-dependent initialisation from this batch (first training forward)
            count = float(N * H * W)
            sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
            L.vqw_actnorm_stats(x, sums, N * H * W, C)  # exact squares: scale = 1 / (std + 1e-6) has no eps to hide behind
            if sync and _dist_on():                    # every rank initialises from the global batch
                _all_reduce(sums)
                count *= dist.get_world_size()
            L.vqw_actnorm_prepare(sums, count, loc, scale, initialized, mrb, C)
        else:
            L.vqw_actnorm_prepare(None, 0.0, loc, scale, None, mrb, C)
        y = torch.empty_like(x, memory_format=CL)
        L.vqw_bn_affine_fwd(x, mrb, scale, mrb[2 * C:], y, N * H * W, C, float(slope))
        ctx.save_for_backward(x, scale, mrb)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, mrb = ctx.saved_tensors
        N, C, H, W = x.shape
        L = _L()
        gy = nhwc(gy)
        mr, beta = mrb, mrb[2 * C:]
        need_params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)     # not read by the eval-form apply without dgamma
        dscale = dbeta = dloc = None
        if need_params:
            ws = _ws(L.vqw_plane_ws_bytes(N, C, H * W), x)
            L.vqw_bn_affine_bwd_reduce(x, mr, scale, beta, gy, sums, ws, ws.numel(), N, H * W, C, ctx.slope)
            dscale = torch.empty((1, C, 1, 1), dtype=torch.float32, device=x.device)
            dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        gx = torch.empty_like(x, memory_format=CL)
        L.vqw_bn_affine_bwd_apply(x, mr, scale, beta, gy, sums, float(N * H * W), gx, dscale, dbeta, N * H * W, C, ctx.slope, 0, 0)
        if need_params:
            dloc = torch.empty((1, C, 1, 1), dtype=torch.float32, device=x.device)
            L.vqw_actnorm_loc_grad(dbeta, scale, dloc, C)
        return gx, dloc, dscale, None, None, None


def act_norm_lrelu(x, loc, scale, initialized=None, slope=0.2, sync=True):
    """ActNorm (logdet=False) followed by nn.LeakyReLU(slope) (slope = 1: plain ActNorm): lrelu(scale * (x + loc)).
    With `initialized` (the module's uint8 flag buffer) loc / scale are first set from this batch - loc = -mean,
    scale = 1 / (unbiased std + 1e-6) per channel, over all ranks when a process group is up - and the flag is raised."""
    return _ActNormLrelu.apply(x, loc, scale, initialized, float(slope), bool(sync))


# pointer tables of the multi-layer launches go up through a small ring of persistent pinned buffers, as hipops.Adam's do
_table_rings = {}


def _upload_table(rows, device):
    import numpy as np
    arr = np.asarray(rows, dtype=np.int64)
    ring = _table_rings.setdefault((device, arr.size), [])
    slot = None
    for cand in ring:
        if cand[1].query():
            slot = cand
            break
    if slot is None:
        if len(ring) >= 8:
            slot = ring[0]
            slot[1].synchronize()
        else:
            slot = [torch.empty(arr.size, dtype=torch.int64).pin_memory(), torch.cuda.Event()]
            ring.append(slot)
    slot[0].numpy()[:] = arr.reshape(-1)
    table = slot[0].to(device, non_blocking=True)
    slot[1].record(torch.cuda.current_stream())
    return table


SN_CHUNK, SN_COLS = 4096, 64         # csrc/spectral.hip


class _SpectralNorm(torch.autograd.Function):
    """weight_i = W_i / sigma_i for n layers at once (csrc/spectral.hip): three launches per forward in training mode, two in
    eval mode, two per backward, whatever n is."""

    @staticmethod
    def forward(ctx, training, eps, n, *ts):
        ws, us, vs, svs = ts[:n], ts[n:2 * n], ts[2 * n:3 * n], ts[3 * n:]       # svs: none, or one per layer (BigGAN's sv0)
        _dev(*ts)
        dev = ws[0].device
        dims = []
        for w, u, v in zip(ws, us, vs):
            rows, cin, kh, kw = w.shape
            K = cin * kh * kw
            if u.numel() != rows or v.numel() != K or u.dtype != torch.float32 or v.dtype != torch.float32:
                raise RuntimeError("spectral_norm_weight: u / v must be fp32 of %d / %d entries for a weight of shape %s"
                                   % (rows, K, tuple(w.shape)))
            if not (u.is_contiguous() and v.is_contiguous()):
                raise RuntimeError("spectral_norm_weight: u / v are updated in place and must be contiguous")
            dims.append((rows, K, cin))
        ws = [nhwc(w) for w in ws]
        outs = [torch.empty(w.shape, dtype=torch.float32, device=dev, memory_format=CL) for w in ws]
        scratch = torch.empty(sum(2 * (rows + K) + 1 for rows, K, _ in dims), dtype=torch.float32, device=dev)
        table, off, b1, b2, b3 = [], scratch.data_ptr(), 0, 0, 0
        saves = []
        for i, (w, u, v, o, (rows, K, cin)) in enumerate(zip(ws, us, vs, outs, dims)):
            save, t, s_ = off, off + 4 * (rows + K + 1), off + 4 * (rows + 2 * K + 1)
            off += 4 * (2 * (rows + K) + 1)
            saves.append(save)
            table.append((w.data_ptr(), u.data_ptr(), v.data_ptr(), o.data_ptr(), save, t, s_, rows, K, cin, b1, b2, b3,
                          svs[i].data_ptr() if svs else 0, 0, 0))
            b1 += -(-K // SN_COLS)
            b2 += rows
            b3 += -(-(rows * K) // SN_CHUNK)
        tab = _upload_table(table, dev)
        _L().vqw_spectral_norm_fwd(tab, n, b1, b2, b3, int(training), float(eps))
        tab.record_stream(torch.cuda.current_stream())
        ctx.save_for_backward(scratch, *outs)
        ctx.cfg = (dims, [sv - scratch.data_ptr() for sv in saves])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        scratch, *outs = ctx.saved_tensors
        dims, save_off = ctx.cfg
        n = len(outs)
        todo = [i for i in range(n) if ctx.needs_input_grad[3 + i] and gs[i] is not None]
        grads = [None] * n
        if todo:
            dev = scratch.device
            chunks = [-(-(dims[i][0] * dims[i][1]) // SN_CHUNK) for i in todo]
            part = torch.empty(sum(chunks), dtype=torch.float64, device=dev)
            table, blk, keep = [], 0, []
            for i, nc in zip(todo, chunks):
                g = nhwc(gs[i])
                keep.append(g)
                grads[i] = torch.empty(outs[i].shape, dtype=torch.float32, device=dev, memory_format=CL)
                table.append((g.data_ptr(), nhwc(outs[i]).data_ptr(), scratch.data_ptr() + save_off[i], grads[i].data_ptr(),
                              part.data_ptr() + 8 * blk, dims[i][0], dims[i][1], blk))
                blk += nc
            tab = _upload_table(table, dev)
            _L().vqw_spectral_norm_bwd(tab, len(todo), blk)
            tab.record_stream(torch.cuda.current_stream())
        return (None, None, None) + tuple(grads) + (None,) * (len(ctx.needs_input_grad) - 3 - n)


def spectral_norm_weights(weight_origs, us, vs, training, eps=1e-12, svs=None, biggan=False):
    """torch.nn.utils.spectral_norm's forward (n_power_iterations=1, dim=0) for a list of conv weights (logical OIHW, OHWI in
    memory) in a number of launches that does not depend on the list's length.  training: v <- normalize(W^T u),
    u <- normalize(W v) in place (no gradient) before sigma = u^T W v; eval: the stored u, v.  -> [W / sigma] as OHWI tensors;
    backward: (G - <G, weight> u v^T) / sigma with the u, v, sigma of that forward.

    biggan=True is the SN of networks/biggan/layers.py:25-94 (one singular vector, one iteration): `us` are the buffers u0
    (1, Cout), `vs` is ignored (v is scratch), `svs` the logging buffers sv0 (1); a 2-D weight (SNLinear) is a (rows, K, 1, 1)
    one.  Every forward iterates; training stores u0 and sv0, eval iterates on a copy and stores nothing."""
    n = len(weight_origs)
    if n == 0:
        return []
    if biggan:
        if svs is None or not (len(us) == len(svs) == n):
            raise RuntimeError("spectral_norm_weights(biggan=True): one u0 and one sv0 per weight")
        _dev(*weight_origs)
        w4 = [w if w.dim() == 4 else w.view(w.shape[0], -1, 1, 1) for w in weight_origs]
        vs = torch.empty(sum(w[0].numel() for w in w4), dtype=torch.float32, device=w4[0].device).split([w[0].numel() for w in w4])
        if not training:
            us = torch.cat([u.reshape(-1) for u in us]).split([u.numel() for u in us])
            svs = ()
        outs = _SpectralNorm.apply(True, float(eps), n, *w4, *us, *vs, *svs)
        return [o.view(w.shape) if w.dim() != 4 else o for o, w in zip(outs, weight_origs)]
    if not (len(us) == len(vs) == n):
        raise RuntimeError("spectral_norm_weights: one u and one v per weight")
    return list(_SpectralNorm.apply(bool(training), float(eps), n, *weight_origs, *us, *vs))


def spectral_norm_weight(weight_orig, u, v, training, eps=1e-12):
    return spectral_norm_weights([weight_orig], [u], [v], training, eps)[0]


# ----------------------------------------------------------------------------------------------
# U-Net discriminator (csrc/unet_dis.hip): block tails, bottleneck head, CutMix, the discriminator half's losses
# ----------------------------------------------------------------------------------------------
class _UNetDownTail(torch.autograd.Function):
    """(out, relu) with out = avgpool2(a) (+ s_low), relu = ReLU(out); one pass each way."""

    @staticmethod
    def forward(ctx, a, s_low, want_out, want_relu):
        _dev(a, s_low)
        a = nhwc(a)
        s_low = nhwc(s_low) if s_low is not None else None
        N, C, H, W = a.shape
        if H % 2 or W % 2:
            raise RuntimeError("unet_down_tail: H and W must be even (got %d x %d)" % (H, W))
        if s_low is not None and tuple(s_low.shape) != (N, C, H // 2, W // 2):
            raise RuntimeError("unet_down_tail: shortcut %s does not match %s at half the size" % (tuple(s_low.shape), tuple(a.shape)))
        out = empty_nhwc(N, C, H // 2, W // 2, a) if want_out else None
        relu = empty_nhwc(N, C, H // 2, W // 2, a) if want_relu else None
        _L().vqw_unet_dtail_fwd(a, s_low, out, relu, N, H, W, C)
        ctx.save_for_backward(relu)
        ctx.cfg = (N, C, H, W, s_low is not None)
        ctx.set_materialize_grads(False)
        return out, relu

    @staticmethod
    def backward(ctx, g_out, g_relu):
        if g_out is None and g_relu is None:
            return (None,) * 4
        (relu,) = ctx.saved_tensors
        N, C, H, W, has_s = ctx.cfg
        g_out = nhwc(g_out) if g_out is not None else None
        g_relu = nhwc(g_relu) if g_relu is not None else None
        need_low = has_s and ctx.needs_input_grad[1]
        like = g_out if g_out is not None else g_relu
        g_full = empty_nhwc(N, C, H, W, like) if ctx.needs_input_grad[0] else None
        g_low = empty_nhwc(N, C, H // 2, W // 2, like) if need_low else None
        if g_full is not None or g_low is not None:
            _L().vqw_unet_dtail_bwd(relu, g_out, g_relu, g_full, g_low, N, H, W, C)
        return g_full, g_low, None, None


def unet_down_tail(a, s_low=None, want_out=True, want_relu=True):
    """DBlock tail (biggan/layers.py:503-506 with AvgPool2d(2)): out = avgpool2(a) (+ s_low) and ReLU(out), the next block's
    conv1 input.  s_low is the 1x1 shortcut evaluated on the pooled block input.  -> (out or None, relu or None)."""
    return _UNetDownTail.apply(a, s_low, bool(want_out), bool(want_relu))


class _UNetUpTail(torch.autograd.Function):
    """(out, cat) with out = h + up2x(s_low) and cat = [ReLU(out) | ReLU(res)] (channel concat), one pass each way."""

    @staticmethod
    def forward(ctx, h, s_low, res, want_out, want_cat):
        _dev(h, s_low, res)
        h, s_low = nhwc(h), nhwc(s_low)
        res = nhwc(res) if res is not None else None
        N, C, H, W = h.shape
        if H % 2 or W % 2 or tuple(s_low.shape) != (N, C, H // 2, W // 2):
            raise RuntimeError("unet_up_tail: shortcut %s does not match %s at half the size" % (tuple(s_low.shape), tuple(h.shape)))
        Cr = 0
        if res is not None:
            if not want_cat or res.shape[0] != N or tuple(res.shape[2:]) != (H, W):
                raise RuntimeError("unet_up_tail: residual %s does not match %s" % (tuple(res.shape), tuple(h.shape)))
            Cr = res.shape[1]
        out = empty_nhwc(N, C, H, W, h) if want_out else None
        cat = empty_nhwc(N, C + Cr, H, W, h) if want_cat else None
        _L().vqw_unet_utail_fwd(h, s_low, res, out, cat, N, H, W, C, Cr)
        ctx.save_for_backward(cat)
        ctx.cfg = (N, C, H, W, Cr)
        ctx.set_materialize_grads(False)
        return out, cat

    @staticmethod
    def backward(ctx, g_out, g_cat):
        if g_out is None and g_cat is None:
            return (None,) * 5
        (cat,) = ctx.saved_tensors
        N, C, H, W, Cr = ctx.cfg
        g_out = nhwc(g_out) if g_out is not None else None
        g_cat = nhwc(g_cat) if g_cat is not None else None
        like = g_out if g_out is not None else g_cat
        g_h = empty_nhwc(N, C, H, W, like)
        g_s = empty_nhwc(N, C, H // 2, W // 2, like)
        g_res = empty_nhwc(N, Cr, H, W, like) if (Cr and g_cat is not None and ctx.needs_input_grad[2]) else None
        _L().vqw_unet_utail_bwd(cat, g_out, g_cat, g_h, g_s, g_res, N, H, W, C, Cr)
        return g_h, g_s, g_res, None, None


def unet_up_tail(h, s_low, res=None, want_out=True, want_cat=True):
    """GBlock2 tail (biggan/layers.py:449-457): out = h + up2x(s_low), s_low the 1x1 shortcut at the low resolution, and the
    rectified concat [ReLU(out) | ReLU(res)] that the next up block's up-sampled 3x3 reads.  -> (out or None, cat or None)."""
    return _UNetUpTail.apply(h, s_low, res, bool(want_out), bool(want_cat))


class _UNetHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, bias):
        _dev(h, w, bias)
        h = nhwc(h)
        N, C, H, W = h.shape
        if w.numel() != C or (bias is not None and bias.numel() != 1):
            raise RuntimeError("unet_bottleneck_head: weight of %d entries for %d channels" % (w.numel(), C))
        w = _flat(w)
        y = torch.empty((N, 1), dtype=torch.float32, device=h.device)
        _L().vqw_unet_head_fwd(h, w, bias, y, N, H * W, C)
        ctx.save_for_backward(h, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        h, w = ctx.saved_tensors
        N, C, H, W = h.shape
        gy = _flat(gy)
        g_h = torch.empty_like(h, memory_format=CL) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        g_b = torch.empty(1, dtype=torch.float32, device=h.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if g_h is not None or g_w is not None or g_b is not None:
            _L().vqw_unet_head_bwd(h, w, gy, g_h, g_w, g_b, N, H * W, C)
        return g_h, g_w, g_b


def unet_bottleneck_head(h, weight, bias=None):
    """linear(sum(relu(h), [2, 3])) with one output (unet_discriminator.py:600-604) -> (N, 1)."""
    return _UNetHead.apply(h, weight, bias)


def _box(box, H, W):
    (y0, y1), (x0, x1) = box
    y0, y1, x0, x1 = int(y0), int(y1), int(x0), int(x1)
    if not (0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
        raise RuntimeError("cutmix rectangle [%d, %d) x [%d, %d) outside %d x %d" % (y0, y1, x0, x1, H, W))
    return y0, y1, x0, x1


def cutmix_select(image, recon, box, flip):
    """mask_src_tgt(image, recon, mask) (utils/__init__.py:216-218) for mask = 1 outside the rectangle box = ((y0, y1), (x0, x1))
    and 0 inside, 1 - mask when `flip`.  No gradient (the reference detaches the result)."""
    _dev(image, recon)
    image, recon = nhwc(image.detach()), nhwc(recon.detach())
    if image.shape != recon.shape:
        raise RuntimeError("cutmix_select: shape mismatch %s vs %s" % (tuple(image.shape), tuple(recon.shape)))
    N, C, H, W = image.shape
    out = torch.empty_like(image, memory_format=CL)
    _L().vqw_cutmix_select(image, recon, out, N, H, W, C, *_box(box, H, W), int(bool(flip)))
    return out


class _UNetDisLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r_map, f_map, c_map, r_b, f_b, c_b, box, flip):
        _dev(r_map, f_map, c_map, r_b, f_b, c_b)
        B, C, H, W = r_map.shape
        if C != 1 or f_map.shape != r_map.shape or c_map.shape != r_map.shape or not (r_b.numel() == f_b.numel() == c_b.numel() == B):
            raise RuntimeError("unet_dis_losses: maps (B, 1, H, W) and bottlenecks (B, 1) expected")
        maps = [nhwc(t) for t in (r_map, f_map, c_map)]
        bots = [_flat(t) for t in (r_b, f_b, c_b)]
        L = _L()
        losses = [torch.empty((), dtype=torch.float32, device=r_map.device) for _ in range(3)]
        ws = _ws(L.vqw_unet_dis_losses_ws_bytes(B * H * W), r_map)
        ctx.cfg = (B, H, W) + _box(box, H, W) + (int(bool(flip)),)
        L.vqw_unet_dis_losses_fwd(*maps, *bots, *losses, ws, ws.numel(), *ctx.cfg)
        ctx.save_for_backward(*maps, *bots)
        ctx.shapes = (r_b.shape, f_b.shape, c_b.shape)
        ctx.set_materialize_grads(False)
        return tuple(losses)

    @staticmethod
    def backward(ctx, g_dis, g_cutmix, g_cons):
        if g_dis is None and g_cutmix is None and g_cons is None:
            return (None,) * 8
        t = ctx.saved_tensors
        gl = [g.contiguous().float() if g is not None else None for g in (g_dis, g_cutmix, g_cons)]
        gm = [torch.empty_like(x, memory_format=CL) for x in t[:3]]
        gb = [torch.empty(sh, dtype=torch.float32, device=t[0].device) for sh in ctx.shapes]
        _L().vqw_unet_dis_losses_bwd(*t, *gl, *gm, *gb, *ctx.cfg)
        return (*gm, *gb, None, None)


def unet_dis_losses(r_map, f_map, cutmix_map, r_bottle, f_bottle, cutmix_bottle, box, flip):
    """(l_dis, l_cutmix, l_consistency) of single_window_trainer.py:324-349 in one pass; the mask is given by the rectangle
    box = ((y0, y1), (x0, x1)) (0 inside, 1 outside) and `flip` (1 - mask).  Gradients reach all six inputs."""
    return _UNetDisLosses.apply(r_map, f_map, cutmix_map, r_bottle, f_bottle, cutmix_bottle, box, bool(flip))


class _Hinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        _dev(x)
        x = x.contiguous() if not (x.is_contiguous() or x.is_contiguous(memory_format=CL)) else x
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        _L().vqw_hinge_fwd(x, x.numel(), mode, loss)
        ctx.save_for_backward(x)
        ctx.mode = mode
        return loss

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = g.contiguous().float()
        _L().vqw_hinge_bwd(x, x.numel(), ctx.mode, g, gx)
        return gx, None


def hinge_real(logits):
    """mean(relu(1 - logits)) (gan_loss.py:7)"""
    return _Hinge.apply(logits, 0)


def hinge_fake(logits):
    """mean(relu(1 + logits)) (gan_loss.py:8)"""
    return _Hinge.apply(logits, 1)


def neg_mean(logits):
    """-mean(logits): the generator loss (single_window_trainer.py:463)"""
    return _Hinge.apply(logits, 2)


def set_conv_backend(mode):
    """0 = auto (MFMA kernels where shapes allow), 1 = generic VALU kernels only (testing), 2 = no LDS-resident tile kernels,
    3 = auto without any Winograd-form kernel (F(2x2, 3x3) forward / input / weight gradients and the nine-product forms of the
    up-sampled layers: plain direct-form arithmetic everywhere).  Modes 2 and 3 are the A/B references of the tests.  Returns
    the previous mode."""
    return _L().vqw_set_conv_backend(int(mode))


# ----------------------------------------------------------------------------------------------
# optional paths: PixelShuffle(2), DropBlock, SoftDice / Focal
# ----------------------------------------------------------------------------------------------
class _PixelShuffle2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _dev(x)
        x = nhwc(x)
        N, C4, h, w = x.shape
        if C4 % 4:
            raise RuntimeError("pixel_shuffle(2): channels must be a multiple of 4")
        y = empty_nhwc(N, C4 // 4, 2 * h, 2 * w, x)
        _L().vqw_pixel_shuffle2(x, y, N, 2 * h, 2 * w, C4 // 4, 0)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = nhwc(gy)
        N, C, H, W = gy.shape
        gx = empty_nhwc(N, 4 * C, H // 2, W // 2, gy)
        _L().vqw_pixel_shuffle2(gy, gx, N, H, W, C, 1)
        return gx


def pixel_shuffle2(x):
    return _PixelShuffle2.apply(x)


def dropblock_mask(seed_mask, block_size):
    """seed (B,H,W) float {0,1} on device -> (keep (B,H,W), scale (1,) = numel/sum(keep))."""
    _dev(seed_mask)
    seed = seed_mask.float().contiguous()
    B, H, W = seed.shape
    keep = torch.empty_like(seed)
    scale = torch.empty(1, dtype=torch.float32, device=seed.device)
    _L().vqw_dropblock_mask(seed, keep, scale, B, H, W, int(block_size))
    return keep, scale


class _DropBlockApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep, scale):
        _dev(x, keep, scale)
        x = nhwc(x)
        N, C, H, W = x.shape
        y = torch.empty_like(x, memory_format=CL)
        _L().vqw_dropblock_apply(x, keep, scale, y, N * H * W, C)
        ctx.save_for_backward(keep, scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        keep, scale = ctx.saved_tensors
        gy = nhwc(gy)
        N, C, H, W = gy.shape
        gx = torch.empty_like(gy, memory_format=CL)
        _L().vqw_dropblock_apply(gy, keep, scale, gx, N * H * W, C)
        return gx, None, None


def dropblock_apply(x, keep, scale):
    return _DropBlockApply.apply(x, keep, scale)


class _SegLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, smooth, gamma, eps):
        _dev(logits, target)
        z = logits.contiguous()
        t = target.float().contiguous()
        if z.dtype != torch.float32 or z.shape != t.shape or z.dim() < 2:
            raise RuntimeError("seg losses: fp32 logits and same-shape one-hot targets (B,C,...) expected")
        B, C = z.shape[0], z.shape[1]
        HW = z.numel() // (B * C)
        L = _L()
        out = torch.empty(2, dtype=torch.float32, device=z.device)
        sums = torch.empty(2 * C + 2, dtype=torch.float64, device=z.device)
        ws = _ws(L.vqw_seg_ws_bytes(C), z)
        L.vqw_seg_losses_fwd(z, t, out, sums, ws, ws.numel(), B, HW, C, ignore_index, smooth, gamma, eps)
        ctx.save_for_backward(z, t, sums)
        ctx.cfg = (ignore_index, smooth, gamma, eps)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_dice, g_focal):
        z, t, sums = ctx.saved_tensors
        ignore_index, smooth, gamma, eps = ctx.cfg
        B, C = z.shape[0], z.shape[1]
        HW = z.numel() // (B * C)
        gz = torch.empty_like(z)
        gd = g_dice.contiguous() if g_dice is not None else None
        gf = g_focal.contiguous() if g_focal is not None else None
        _L().vqw_seg_losses_bwd(z, t, sums, gd, gf, gz, B, HW, C, ignore_index, smooth, gamma, eps)
        return gz, None, None, None, None, None


def seg_losses(logits, target, ignore_index=-1, smooth=1e-6, gamma=2.0, eps=1e-6):
    """-> (soft dice loss, focal loss) of functions/seg_loss.py for NCHW logits and one-hot targets."""
    return _SegLosses.apply(logits, target, int(ignore_index), float(smooth), float(gamma), float(eps))


# ----------------------------------------------------------------------------------------------
# 8-bit export (csrc/export.hip): grey tiles through display windows, id maps as index / RGB planes and counts
# ----------------------------------------------------------------------------------------------
EXPORT_MAX_WINDOWS = 8
EXPORT_MAX_DICT_SIZE = 65535
_export_tables = {}
_palettes = {}


def default_palette(dict_size):
    """(K + 1, 3) uint8 numpy palette for ids 0..K: matplotlib's 'Spectral' colour map (the reference's CMAP) sampled at
    K + 1 evenly spaced points when matplotlib imports, otherwise a fixed blue-to-red hue ramp of this project."""
    import numpy as np
    K = int(dict_size)
    pal = _palettes.get(K)
    if pal is None:
        try:
            import matplotlib
            cmap = matplotlib.colormaps["Spectral"] if hasattr(matplotlib, "colormaps") else None
            if cmap is None:
                from matplotlib import cm
                cmap = cm.get_cmap("Spectral")
            pal = (np.asarray(cmap(np.linspace(0.0, 1.0, K + 1)))[:, :3] * 255.0 + 0.5).astype(np.uint8)
        except Exception:
            t = np.linspace(0.0, 1.0, K + 1)
            pal = np.stack([255.0 * t, 255.0 * (1.0 - np.abs(2.0 * t - 1.0)), 255.0 * (1.0 - t)], axis=1)
            pal = (pal + 0.5).astype(np.uint8)
        _palettes[K] = pal = np.ascontiguousarray(pal)
    return pal


def _export_window_rows(windows, vmin, vmax):
    import numpy as np
    if not float(vmax) > float(vmin):
        raise ValueError("export_grey: vmax must be greater than vmin (got %r, %r)" % (vmin, vmax))
    if not 1 <= len(windows) <= EXPORT_MAX_WINDOWS:
        raise ValueError("export_grey: 1..%d windows (got %d)" % (EXPORT_MAX_WINDOWS, len(windows)))
    lo32 = np.float32(vmin)
    rows = []
    for w in windows:
        w = _IDENTITY_WINDOW if w is None else tuple(float(v) for v in w)
        if len(w) != 4:
            raise ValueError("export_grey: a window is None or (alpha, beta, lo, hi) as ops.window_map returns it")
        rows.append(w + (float(lo32), float(np.float32(vmax) - lo32)))
    return tuple(rows)


def export_grey(x, windows=(None,), vmin=-1.0, vmax=1.0, flip=False):
    """(B, 1, H, W) fp32 images (either memory format) -> (n_windows, B, H, W) uint8 tiles,
    u8 = min(255, floor(256 * clamp((w(x) - vmin) / (vmax - vmin), 0, 1))), w = the identity (None) or the window map
    (alpha, beta, lo, hi) of ops.window_map: x -> clamp(alpha * x + beta, lo, hi).  One float32 rounding per operation.
    All windows come from one read of x; flip=True writes the rows bottom to top (np.flipud per image)."""
    windows = tuple(windows)
    rows = _export_window_rows(windows, vmin, vmax)
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise RuntimeError("export_grey: expected an fp32 tensor (got %s)" % (getattr(x, "dtype", type(x)),))
    if x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError("export_grey: expected a (B, 1, H, W) tensor, got shape %s" % (tuple(x.shape),))
    if x.numel() == 0:
        raise RuntimeError("export_grey: empty input")
    _dev(x)
    x = x.detach()
    B, _, H, W = x.shape
    x = x.reshape(B, H, W).contiguous()                # one channel: NCHW and NHWC hold the same bytes, no copy
    key = (x.device, rows)
    tab = _export_tables.get(key)
    if tab is None:
        tab = torch.tensor(rows, dtype=torch.float32).to(x.device)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()
        _export_tables[key] = tab
    out = torch.empty((len(rows), B, H, W), dtype=torch.uint8, device=x.device)
    _L().vqw_export_grey(x, tab, out, len(rows), B, H, W, int(bool(flip)))
    return out


def export_grey_auto(x, flip=False, return_range=False):
    """(B, 1, H, W) fp32 images (either memory format) -> (B, H, W) uint8 tiles, each image over its own range (imshow with
    vmin = vmax = None): u8 = min(255, floor(256 * clamp((x - vmin_b) / (vmax_b - vmin_b), 0, 1))) with vmin_b / vmax_b the
    minimum / maximum over the finite values of image b; one float32 rounding per operation.  Non-finite values, a constant
    image and an image without a finite value export as 0.  flip=True writes the rows bottom to top.  return_range=True ->
    (tiles, (B, 2) fp32 (vmin_b, vmax_b); (+inf, -inf) where an image has no finite value)."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise RuntimeError("export_grey_auto: expected an fp32 tensor (got %s)" % (getattr(x, "dtype", type(x)),))
    if x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError("export_grey_auto: expected a (B, 1, H, W) tensor, got shape %s" % (tuple(x.shape),))
    if x.numel() == 0:
        raise RuntimeError("export_grey_auto: empty input")
    _dev(x)
    x = x.detach()
    B, _, H, W = x.shape
    x = x.reshape(B, H, W).contiguous()                # one channel: NCHW and NHWC hold the same bytes, no copy
    L = _L()
    out = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
    rng = torch.empty((B, 2), dtype=torch.float32, device=x.device) if return_range else None
    ws = _ws(L.vqw_export_auto_ws_bytes(B), x)
    L.vqw_export_grey_auto(x, out, rng, ws, ws.numel(), B, H, W, int(bool(flip)))
    return (out, rng) if return_range else out


class LabelExport:
    """Result of ops.export_labels: device tensors `index` (B, H, W) uint8 / uint16, `rgb` (B, H, W, 3) uint8 and `counts`
    (B, K + 1) int32 (each None when not asked for).  check() reads the error flag (one small device-to-host copy) and
    raises ValueError when an id lay outside [0, dict_size]."""

    def __init__(self, index, rgb, counts, err):
        self.index, self.rgb, self.counts, self._err = index, rgb, counts, err

    def check(self):
        if self._err is not None:
            bad = int(self._err.cpu()[0])
            self._err = None
            if bad:
                raise ValueError("export_labels: ids outside [0, dict_size]")
        return self


def export_labels(ids, dict_size, palette=None, index=True, rgb=True, counts=True, flip=False, check=True):
    """ids (B, H, W) int64 in [0, K] -> LabelExport(index plane, RGB plane through `palette` ((K + 1, 3) uint8; default
    ops.default_palette), per-image counts of ids 0..K).  flip=True writes rows bottom to top.  With check=True (default)
    an id outside [0, K] raises ValueError here, which reads the flag to the host; check=False leaves that to .check()."""
    K = int(dict_size)
    if not 1 <= K <= EXPORT_MAX_DICT_SIZE:
        raise ValueError("export_labels: dict_size must be in [1, %d] (got %d)" % (EXPORT_MAX_DICT_SIZE, K))
    if not torch.is_tensor(ids) or ids.dtype != torch.int64:
        raise RuntimeError("export_labels: ids must be an int64 tensor (got %s)" % (getattr(ids, "dtype", type(ids)),))
    if ids.dim() != 3:
        raise RuntimeError("export_labels: expected (B, H, W) ids, got shape %s" % (tuple(ids.shape),))
    if ids.numel() == 0:
        raise RuntimeError("export_labels: no ids")
    if rgb:
        import numpy as np
        if palette is None:
            palette = default_palette(K)
        if torch.is_tensor(palette):
            if palette.dtype != torch.uint8 or tuple(palette.shape) != (K + 1, 3):
                raise ValueError("export_labels: the palette must be (%d, 3) uint8 (got %s %s)"
                                 % (K + 1, tuple(palette.shape), palette.dtype))
        else:
            palette = np.asarray(palette)
            if palette.dtype != np.uint8 or palette.shape != (K + 1, 3):
                raise ValueError("export_labels: the palette must be (%d, 3) uint8 (got %s %s)"
                                 % (K + 1, palette.shape, palette.dtype))
    _dev(ids)
    ids = ids.detach().contiguous()                    # the encoder's ids are a transposed view: the planes need rows
    dev = ids.device
    B, H, W = ids.shape
    pal_dev = None
    if rgb:
        if torch.is_tensor(palette):
            pal_dev = palette.to(dev).contiguous()
        else:
            key = (dev, K, palette.tobytes())
            pal_dev = _export_tables.get(key)
            if pal_dev is None:
                pal_dev = torch.from_numpy(np.ascontiguousarray(palette)).to(dev)
                if not torch.cuda.is_current_stream_capturing():
                    torch.cuda.current_stream().synchronize()
                _export_tables[key] = pal_dev
    idx_t = torch.empty((B, H, W), dtype=torch.uint8 if K <= 255 else torch.uint16, device=dev) if index else None
    rgb_t = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if rgb else None
    cnt_t = torch.empty((B, K + 1), dtype=torch.int32, device=dev) if counts else None
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _L().vqw_export_labels(ids, pal_dev, idx_t, rgb_t, cnt_t, err, B, H, W, K, int(bool(flip)))
    res = LabelExport(idx_t, rgb_t, cnt_t, err)
    return res.check() if check else res


# ---- preprocessing: NIfTI volumes -> slice datasets (csrc/resample.hip) -------------------------------------------------
VOLUME_DTYPES = {"uint8": 0, "int16": 1, "uint16": 2, "int32": 3, "float32": 4, "float64": 5}
NORMS = {None: 0, "minmax": 1, "zscore": 2}
ORIENTATIONS = {None: 0, "crc": 1, "brats": 2}        # crc: np.rot90(s[::-1]); brats: np.rot90(s, k=3)
_resample_tables = {}


def bilinear_coefficients(in_size, out_size):
    """PIL's precompute_coeffs for its bilinear filter (support 1) over the whole axis, in double: -> (k [out][ksize]
    float64 normalised coefficients, bounds [out][2] int32 = first tap, tap count).  The filter argument is formed as
    (x - center + 0.5) * (1.0 / filterscale), the reciprocal taken once, as PIL does."""
    import numpy as np
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.abs((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        w = np.where(w < 1.0, 1.0 - w, 0.0)
        ww = 0.0
        for v in w:                                   # PIL's running sum, in index order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        k[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    return k, bounds


def nearest_indices(in_size, out_size):
    """Source index of every output pixel of PIL's NEAREST resize: PIL steps a double coordinate, xo = 0.5 * scale, then
    xo += scale per pixel, and truncates it (equal to floor((i + 0.5) * in / out) wherever that running sum is exact)."""
    import numpy as np
    scale = float(in_size) / float(out_size)
    idx = np.empty(out_size, dtype=np.int32)
    xo = 0.0 + scale * 0.5
    for i in range(out_size):
        idx[i] = min(int(xo), in_size - 1)
        xo += scale
    return idx


def _resample_table(kind, in_size, out_size, device):
    key = (kind, int(in_size), int(out_size), device)
    tab = _resample_tables.get(key)
    if tab is None:
        if kind == "bilinear":
            k, b = bilinear_coefficients(int(in_size), int(out_size))
            tab = (torch.from_numpy(k).to(device), torch.from_numpy(b).to(device), k.shape[1])
        else:
            tab = torch.from_numpy(nearest_indices(int(in_size), int(out_size))).to(device)
        torch.cuda.current_stream().synchronize()
        _resample_tables[key] = tab
    return tab


def _volume_arg(vol, name):
    if not torch.is_tensor(vol):
        raise RuntimeError("%s: expected a tensor (got %s)" % (name, type(vol)))
    code = VOLUME_DTYPES.get(str(vol.dtype).replace("torch.", ""))
    if code is None:
        raise RuntimeError("%s: the volume must be one of %s (got %s)" % (name, ", ".join(VOLUME_DTYPES), vol.dtype))
    if vol.dim() != 3 or vol.numel() == 0:
        raise RuntimeError("%s: expected a non-empty (Z, Y, X) volume, got shape %s" % (name, tuple(vol.shape)))
    _dev(vol)
    return vol.detach().contiguous(), code


def _scaling(slope, inter):
    """nibabel applies scl_slope / scl_inter unless they are the identity; a slope of 0 means 'not set'."""
    slope, inter = float(slope), float(inter)
    if slope == 0.0:
        slope = 1.0
    return slope, inter, int(slope != 1.0 or inter != 0.0)


def volume_stats(vol, slope=1.0, inter=0.0):
    """vol: (Z, Y, X) device tensor in the dtype the file stores (the NIfTI array with its axes reversed, so x is the
    fastest) -> (5,) float64 device tensor: min, max of value = double(stored) [* slope + inter], then count, mean and
    population standard deviation of the float32(value) > 0, summed in double in a fixed order (bit-identical run to run)."""
    vol, code = _volume_arg(vol, "volume_stats")
    slope, inter, scaled = _scaling(slope, inter)
    L = _L()
    stats = torch.empty(5, dtype=torch.float64, device=vol.device)
    ws = torch.empty(int(L.vqw_volume_stats_ws_bytes()) // 8, dtype=torch.float64, device=vol.device)
    L.vqw_volume_stats(vol, stats, ws, code, vol.numel(), slope, inter, scaled)
    return stats


def volume_to_slices(vol, size, norm=None, orient=None, stats=None, slope=1.0, inter=0.0):
    """vol (Z, Y, X) as volume_stats takes it -> (Z, size, size) float32: every slice normalised (norm 'minmax': ((v - min) /
    (max - min)) * 255 in double, rounded once to float32; 'zscore': (float32(v) - mean32) / std32; None: float32(v)),
    oriented (orient 'crc': np.rot90(s[::-1]); 'brats': np.rot90(s, k=3); None: s[x, y]) and resized like PIL's
    Image.resize((size, size), BILINEAR) in mode F, bit for bit.  stats: ops.volume_stats of the volume (computed here when a
    normalisation needs it and none is given)."""
    if norm not in NORMS or orient not in ORIENTATIONS:
        raise ValueError("volume_to_slices: norm is one of %s, orient one of %s" % (sorted(map(str, NORMS)), sorted(map(str, ORIENTATIONS))))
    S = int(size)
    if S < 1:
        raise ValueError("volume_to_slices: size must be positive (got %d)" % S)
    n, o = NORMS[norm], ORIENTATIONS[orient]
    vol, code = _volume_arg(vol, "volume_to_slices")
    if n and stats is None:
        stats = volume_stats(vol, slope, inter)
    if stats is not None:
        _dev(stats)
        if stats.dtype != torch.float64 or stats.numel() != 5:
            raise RuntimeError("volume_to_slices: stats is the (5,) float64 tensor of ops.volume_stats")
        stats = stats.contiguous()
    slope, inter, scaled = _scaling(slope, inter)
    Z, Y, X = vol.shape
    h, w = (X, Y) if o == 0 else (Y, X)
    dev = vol.device
    kh, bh, ksh = _resample_table("bilinear", w, S, dev) if w != S else (None, None, 0)
    kv, bv, ksv = _resample_table("bilinear", h, S, dev) if h != S else (None, None, 0)
    tmp = torch.empty((Z, h, S), dtype=torch.float32, device=dev) if ksv else None
    out = torch.empty((Z, S, S), dtype=torch.float32, device=dev)
    _L().vqw_volume_to_slices(vol, stats, kh, bh, kv, bv, tmp, out, code, X, Y, Z, S, ksh, ksv, n, o, slope, inter, scaled)
    return out


def label_volume_to_slices(vol, size, orient=None, relabel=False):
    """vol (Z, Y, X) int32 labels -> (Z, size, size) int32: every oriented slice resized like PIL's NEAREST.  relabel=True is
    the BraTS training relabel 4 -> 3, and raises ValueError when a voxel of the volume already carries label 3 (the
    reference's assertion; one small device-to-host copy)."""
    if not torch.is_tensor(vol) or vol.dtype != torch.int32:
        raise RuntimeError("label_volume_to_slices: labels must be an int32 tensor (got %s)" % (getattr(vol, "dtype", type(vol)),))
    if orient not in ORIENTATIONS:
        raise ValueError("label_volume_to_slices: orient is one of %s" % sorted(map(str, ORIENTATIONS)))
    S = int(size)
    if S < 1:
        raise ValueError("label_volume_to_slices: size must be positive (got %d)" % S)
    o = ORIENTATIONS[orient]
    vol, _ = _volume_arg(vol, "label_volume_to_slices")
    Z, Y, X = vol.shape
    h, w = (X, Y) if o == 0 else (Y, X)
    dev = vol.device
    xtab = _resample_table("nearest", w, S, dev)
    ytab = _resample_table("nearest", h, S, dev)
    out = torch.empty((Z, S, S), dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _L().vqw_label_slices(vol, xtab, ytab, out, err, X, Y, Z, S, o, int(bool(relabel)))
    if relabel and int(err.cpu()[0]):
        raise ValueError("label_volume_to_slices: the volume already carries label 3; 4 -> 3 would merge two classes")
    return out
