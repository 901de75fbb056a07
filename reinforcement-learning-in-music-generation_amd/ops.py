"""Python bindings of the libcwlt kernels: raw launch wrappers + torch.autograd Functions.

Everything here runs on the GPU through the C-ABI in include/cwlt.h; there is no CPU path.
"""
import ctypes
import math
import os

import torch

from . import _lib

CLA_EPS = 1e-6  # fast_transformers CausalLinearAttention default eps
LN_EPS = 1e-5   # nn.LayerNorm default, used by fast_transformers' encoder layers


# --------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------
def _row_stride(t):
    """Row stride of an (N, L, H, D) or (R, H, D) view of a row buffer whose last two dims are dense and (4-D) whose batch
    stride is L*row_stride; None where the kernels cannot take the view as it is."""
    H, D = t.shape[-2:]
    if t.numel() == 0:
        return H * D                 # empty batch / sequence: strides are irrelevant
    if t.stride(-1) != 1 or t.stride(-2) != D:
        return None
    ld = t.stride(-3)
    if t.dim() == 4 and t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld:
        return None
    if ld % 4 != 0 or t.data_ptr() % 16 != 0:
        return None
    return ld


def _as_rows(t):
    ld = _row_stride(t)
    if ld is None:
        t = t.contiguous()
        ld = _row_stride(t)
    return t, ld


def _f32(t):
    """Parameter as a dense f32 device tensor (the kernels read gamma/beta/bias/tables in f32)."""
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (torch's current stream).

    bench.py switches it on for the timed region; each C-ABI call is then bracketed by two events.
    `summary()` (after a device sync) -> {entry point: (calls, mean ms)}."""
    enabled = False
    records = {}
    pool = []

    @classmethod
    def reset(cls, enabled):
        cls.enabled = bool(enabled)
        cls.records = {}

    @classmethod
    def reserve(cls, n):
        """Create (and once record) n timing events ahead of the timed region: hipEventCreate is slow, and the
        first few hundred creations are the slowest."""
        while len(cls.pool) < n:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            cls.pool.append(e)

    @classmethod
    def event(cls):
        return cls.pool.pop() if cls.pool else torch.cuda.Event(enable_timing=True)

    @classmethod
    def summary(cls):
        """{entry point: (calls, mean ms, mean work per call or None)} -- `work` is what the caller declared for
        the launch (FLOPs of a weight-gradient GEMM of that very shape), so rates use the real per-call shapes."""
        out = {}
        for name, evs in cls.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in evs]
            works = [w for _, _, w in evs if w is not None]
            out[name] = (len(ms), sum(ms) / max(1, len(ms)), (sum(works) / len(works)) if works else None)
        return out


def _call(name, *args, work=None):
    """Invoke one libcwlt entry point on the current stream and raise on a non-zero status."""
    fn = getattr(_lib.load(), name)
    if KernelTimer.enabled:
        a, b = KernelTimer.event(), KernelTimer.event()
        a.record()
        st = fn(*args)
        b.record()
        KernelTimer.records.setdefault(name, []).append((a, b, work))
    else:
        st = fn(*args)
    _lib.check(st, name)


def direct_grads(param=None):
    """True when parameter gradients may be written straight into .grad by the layer backward: always in a
    single process; under data parallelism only for parameters owned by a `dist.GradSync` (it is told through
    the parameter's `_cwlt_ready` callback) -- with any other gradient hook (e.g. DDP) gradients go through
    autograd so that the hooks fire."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return True
    return param is not None and getattr(param, "_cwlt_ready", None) is not None


def deliver_grad(p, g):
    """p.grad += g with one fused convert + add (g may be bf16, p.grad is f32)."""
    if not p.requires_grad:
        return
    if p.grad is None:
        p.grad = g.float().clone() if g.dtype == torch.float32 else g.float()
    else:
        p.grad.add_(g)


def deliver_grads(pairs):
    """deliver_grad for a list of (parameter, gradient) pairs with ONE multi-tensor launch instead of one small
    device op per parameter (16 per encoder layer, ~9 us each).  Always an accumulation, as autograd's own
    AccumulateGrad: the buffers are zeroed by zero_grad().
    Never allocates while a hipGraph is being captured: a captured step must find every `.grad` in place (the flat
    buckets of dist.GradSync) -- a gradient tensor created inside the capture would live in the graph's private
    pool while `.grad` kept pointing at it from outside; that is refused here instead of being left to chance."""
    dst, src = [], []
    for p, g in pairs:
        if not p.requires_grad:
            continue
        if p.grad is None:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("deliver_grads under graph capture: a parameter has no .grad buffer yet -- attach "
                                   "the gradients (dist.GradSync) and run the step eagerly once before capturing it")
            p.grad = g.float().clone() if g.dtype == torch.float32 else g.float()
        else:
            dst.append(p.grad)
            src.append(g.view(p.grad.shape) if g.dtype == p.grad.dtype else g.view(p.grad.shape).to(p.grad.dtype))
    if dst:
        torch._foreach_add_(dst, src)
    for p, _ in pairs:                       # data parallel: tell the gradient buckets (dist.GradSync)
        ready = getattr(p, "_cwlt_ready", None)
        if ready is not None and p.requires_grad:
            ready(p)


def deliver_grads_flat(params, grads, all_need_grad):
    """deliver_grads for a cached flat parameter list and its gradient views (encoder._EncoderStackFn): no per-pair
    Python work on the common path (every parameter trainable and already holding a .grad buffer)."""
    dst = [q.grad for q in params]
    if not all_need_grad or any(g is None for g in dst):
        return deliver_grads(list(zip(params, grads)))
    torch._foreach_add_(dst, grads)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for q in params:
            ready = getattr(q, "_cwlt_ready", None)
            if ready is not None:
                ready(q)


_seed_counter = [0]


def next_seed():
    """Fresh 62-bit dropout key from torch's CPU generator (reproducible under torch.manual_seed)."""
    _seed_counter[0] += 1
    return int(torch.empty((), dtype=torch.int64).random_().item()) & ((1 << 62) - 1)


def next_seeds(k):
    """k dropout keys in one draw: the same values as k calls of next_seed() (one generator call per element, in order)."""
    _seed_counter[0] += k
    return [v & ((1 << 62) - 1) for v in torch.empty(k, dtype=torch.int64).random_().tolist()]


# A captured hipGraph bakes every kernel argument, dropout seeds included.  The dropout kernels therefore accept
# an optional device pointer to one uint64 that is ADDED to the seed when the kernel runs (include/cwlt.h,
# "seed_base").  It is passed only while `GraphedCall` captures (and warms up) a function; the captured graph
# starts by bumping the value, so every replay draws fresh masks.  Eager launches pass NULL.
_SEED_BASE = {}
_USE_SEED_BASE = False
_SEED_STEP = 0x9E3779B97F4A7C15 - (1 << 64)     # golden-ratio increment as a signed 64-bit integer


def seed_base_tensor(device=None):
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    t = _SEED_BASE.get(idx)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("seed base must exist before graph capture starts")
        t = torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", idx))
        _SEED_BASE[idx] = t
    return t


def _seed_base():
    return _lib.dev(seed_base_tensor()) if _USE_SEED_BASE else None


GRAPHS_ENABLED = os.environ.get("CWLT_GRAPHS", "1") != "0"     # CWLT_GRAPHS=0: RL rollout / update steps launch eagerly


TRAIN_GRAPHS = os.environ.get("CWLT_TRAIN_GRAPHS", "0") == "1"


def train_graphs_enabled():
    """Whole-training-step graphs (forward + backward + Adam of DQN.update / PPO.update_policy in one launch): OPT-IN
    with CWLT_TRAIN_GRAPHS=1 (and not CWLT_GRAPHS=0), single process only (under data parallelism the gradient
    all-reduce stays eager).  The no-grad rollout graphs (GRAPHS_ENABLED) are unaffected and on by default.

    Why opt-in: in round 1 a captured DQN.update produced NaN losses from its third replay on --
    once hipErrorIllegalAddress -- whenever large eager GEMMs ran between replays.  The change that made it go away
    (accumulate-only gradient delivery instead of copy-on-first-delivery) is arithmetically equivalent to what it
    replaced and explains neither symptom; in round 2 neither the old delivery re-created on the current tree
    (tools/diag_fresh_copy.py) nor the tree that preceded the change, run with its own failing recipe, reproduces
    the fault on this round's boxes (gpurun_out/r02_diag_*.log).  The cause is therefore NOT known.  What is in
    place instead of a diagnosis: captured steps never allocate gradient storage (deliver_grads), a captured step
    checks on every replay that the gradient / parameter storage it was captured against is still where it was
    (GraphedCall(params=...)), and the feature stays off unless asked for."""
    import torch.distributed as dist
    single = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
    return GRAPHS_ENABLED and TRAIN_GRAPHS and single


FUSED_ADAM = os.environ.get("CWLT_FUSED_ADAM", "1") != "0"


def graph_adam(params, lr, **kw):
    """torch.optim.Adam as the reference constructs it; when training steps may be captured, `capturable=True`
    with the learning rate held in a device tensor, so an LR scheduler's updates reach the captured step.
    `fused=True` there: the capturable multi-tensor ("foreach") path divides every state tensor by 0-dim tensors one
    parameter at a time (2 x 438 launches per PPO step, 14 % of the window-50 update's GPU time); the fused kernel
    does the whole step in a few launches."""
    params = list(params)
    if train_graphs_enabled() and params and params[0].is_cuda:
        return torch.optim.Adam(params, lr=torch.tensor(float(lr), device=params[0].device), capturable=True,
                                fused=True, **kw)
    # eager steps: the single-kernel ("fused") implementation of the same update -- the default multi-tensor one is
    # eight passes over every parameter and state tensor per step (9 % of the GPU time of a window-50 PPO iteration,
    # profiles/r04_ppo_w50_kernels.txt).  CWLT_FUSED_ADAM=0: torch's default implementation.
    if FUSED_ADAM and params and all(q.is_cuda and q.dtype == torch.float32 for q in params):
        return torch.optim.Adam(params, lr=lr, fused=True, **kw)
    return torch.optim.Adam(params, lr=lr, **kw)


def capture_hip_graph(body, mode=torch.no_grad, name="step"):
    """Capture `body()` on the current stream into a hipGraph that is safe to replay on this runtime.
    -> (torch.cuda.CUDAGraph or None, body's result, node census before the rewrite, memset nodes rewritten).

    A captured hipMemsetAsync replays a WRONG fill pattern on ROCm 7.2 from the second replay on when other work runs
    in between (tools/probes/graph_memset_probe.py), and library code inside a captured step issues such memsets
    (PyTorch's reduction semaphores, hipBLASLt's split-K workspaces: tools/diag_memset_sites.py).  Before the graph is
    instantiated every memset node is therefore replaced by a fill-kernel node (cwlt_graph_replace_memset_nodes).
    keep_graph: the hipGraph_t stays accessible after the capture so that its nodes can be counted and edited; the
    executable graph is instantiated by the first replay.  Should any memset node remain (inside a child graph), None
    is returned in place of the graph: the caller must run the step eagerly -- the capture itself executed nothing."""
    import warnings
    if not _graph_editing_available():
        # a PyTorch without CUDAGraph(keep_graph=True) / raw_cuda_graph(): the graph's nodes can be neither counted nor
        # rewritten, so nothing is captured and the caller runs the step eagerly (one warning per process)
        if not _GRAPH_API[1]:
            _GRAPH_API[1] = True
            warnings.warn("capture_hip_graph: this PyTorch has no CUDAGraph(keep_graph=True).raw_cuda_graph(); "
                          "hipGraph capture is off, steps run eagerly")
        return None, None, {}, 0
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    # No cyclic garbage collection while the stream captures.  A collection that starts inside the capture (in this
    # thread or in autograd's) may reach a dead cycle that still holds an earlier hipGraph -- a GraphedCall and the
    # object whose bound method it wraps, say; torch.cuda.graph no longer collects before it begins -- and a CUDAGraph's
    # destructor synchronises the device on ROCm, which a capture in the global error mode turns into an error thrown
    # from a destructor: the process aborts.  Such garbage waits for the first collection after the capture.
    import gc
    collecting = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph), mode():
            out = body()
    finally:
        if collecting:
            gc.enable()
    raw = graph.raw_cuda_graph()
    census = _lib.graph_node_census(raw)
    replaced = 0
    if census.get("memset", 0):
        n = ctypes.c_int(0)
        st = _lib.load().cwlt_graph_replace_memset_nodes(ctypes.c_void_p(int(raw)), ctypes.byref(n))
        replaced = n.value
        left = -1 if st else _lib.graph_node_census(raw).get("memset", 0)
        if left:
            # a rewrite that failed (status != 0: e.g. an element size the fill kernel does not take) or left a node
            # inside a child graph: the step runs eagerly rather than raising out of a training loop
            warnings.warn("capture_hip_graph: the captured %s %s (%s); a replayed hipMemsetAsync is not reliable on this "
                          "runtime -- running it eagerly instead"
                          % (name, "could not be rewritten (status %d)" % st if st
                             else "still holds %d memset node(s) after the rewrite" % left, census))
            graph.reset()
            graph = None
    return graph, out, census, replaced


_GRAPH_API = [None, False]          # [keep_graph / raw_cuda_graph available, warned]


def _graph_editing_available():
    if _GRAPH_API[0] is None:
        try:
            import inspect
            ok = hasattr(torch.cuda.CUDAGraph, "raw_cuda_graph")
            if ok:
                try:
                    ok = "keep_graph" in inspect.signature(torch.cuda.CUDAGraph.__new__).parameters
                except (TypeError, ValueError):
                    ok = True                      # signature not introspectable: trust the method's presence
            _GRAPH_API[0] = bool(ok)
        except Exception:
            _GRAPH_API[0] = False
    return _GRAPH_API[0]


class GraphedCall:
    """Run `fn(*tensors)` -- a sync-free function of device tensors -- as ONE hipGraph launch.

    grad=False: a no-grad forward (an RL rollout step: trunk forward + heads + action gather, a few hundred launches
    for a 50-token window).  Warmed up on a side stream, then captured on the first call.
    grad=True: a whole training step -- forward, backward and optimizer.step() (optimizers built with
    capturable=True) -- for the launch-bound small-batch updates of the RL loops.  The first `eager_calls` calls
    run eagerly (they are real steps and create the optimizer state); the next call is captured, then replayed.

    Captured once per input signature; replays copy the arguments into the graph's static inputs, bump the dropout
    seed base (a captured op) and launch.  Parameters, gradients and optimizer state are used in place.
    Outputs are the graph's static buffers: valid until the next call with the same signature."""

    def __init__(self, fn, warmup=2, grad=False, eager_calls=2, params=None):
        self.fn, self.warmup, self.grad, self.eager_calls = fn, warmup, grad, eager_calls
        self.graphs, self.calls = {}, {}
        self.census = None                                 # node kinds of the last capture (_lib.graph_node_census)
        self.memsets_replaced = 0
        # grad=True: the parameters the step trains.  Their storage and their .grad storage are baked into the graph
        # as raw addresses; `_storage()` is compared before every replay so that a moved buffer (a dropped / re-made
        # .grad, a re-allocated parameter) raises instead of letting the graph write through a stale address.
        self.params = [p for p in params if p.requires_grad] if params is not None else None
        self._addr = {}

    def _storage(self):
        if not self.params:
            return None
        if any(p.grad is None for p in self.params):
            raise RuntimeError("GraphedCall(grad=True): a trained parameter has no .grad buffer -- gradients must live "
                               "in persistent storage (dist.GradSync buckets) before the step is captured")
        return tuple((p.data_ptr(), p.grad.data_ptr()) for p in self.params)

    def _capture(self, args):
        global _USE_SEED_BASE
        dev = args[0].device
        base = seed_base_tensor(dev)
        static = [a.clone() for a in args]
        was_timing = KernelTimer.enabled
        KernelTimer.enabled = False
        _USE_SEED_BASE = True
        mode = torch.enable_grad if self.grad else torch.no_grad
        try:
            if not self.grad:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side), torch.no_grad():
                    for _ in range(self.warmup):
                        self.fn(*static)
                torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            before = self._storage()
            def body():
                base.add_(_SEED_STEP)
                return self.fn(*static)
            graph, out, self.census, self.memsets_replaced = capture_hip_graph(
                body, mode, getattr(self.fn, "__name__", "step"))
            if self._storage() != before:
                raise RuntimeError("GraphedCall(grad=True): parameter / gradient storage changed DURING capture")
        finally:
            _USE_SEED_BASE = False
            KernelTimer.enabled = was_timing
        return graph, static, out

    def __call__(self, *args):
        key = tuple((tuple(a.shape), a.dtype, a.device.index) for a in args)
        ent = self.graphs.get(key)
        if ent is None:
            n = self.calls.get(key, 0)
            if self.grad and n < self.eager_calls:
                self.calls[key] = n + 1
                return self.fn(*args)
            ent = self.graphs[key] = self._capture(args)
            self._addr[key] = self._storage()
        graph, static, out = ent
        if graph is None:                                  # a capture that was refused (memset nodes): eager
            return self.fn(*args)
        if self.params and self._storage() != self._addr[key]:
            raise RuntimeError("GraphedCall(grad=True): parameter / gradient storage moved since the step was "
                               "captured (a .grad was dropped or re-created, or a parameter re-allocated)")
        for s, a in zip(static, args):
            s.copy_(a)
        graph.replay()
        return out



# --------------------------------------------------------------------------------------------------
# compute-dtype copies of the master parameters
# --------------------------------------------------------------------------------------------------
# The f32 master weights are used in bf16 (and Q/K/V row-stacked) by every layer.  Casting them per call is seven
# 1-4 MB copy kernels + two cat kernels per layer per forward: nothing at B*T = 524 288 rows, but a third of the GPU
# time of the launch-bound RL steps (window 50: 108 such kernels per 12-layer trunk forward).  A ShadowSet keeps
# persistent copies and refreshes ALL of them with one multi-tensor copy per forward.
#
# The refresh is unconditional: nothing cheap says whether a parameter changed (fused optimizers and replays of a
# captured optimizer step move parameters WITHOUT bumping autograd's version counters).  Only inside
# `with ops.frozen_weights():` -- a scope in which the caller guarantees that no parameter changes, e.g. the loop
# over buffer batches of one reward-scoring call -- is a set refreshed once and then reused.
_FROZEN = [0]            # id of the innermost frozen_weights scope, 0 outside any
_FROZEN_IDS = [0]


class frozen_weights:
    """Scope in which no parameter of any model changes: ShadowSets refresh at most once inside it."""

    def __enter__(self):
        self.prev = _FROZEN[0]
        _FROZEN_IDS[0] += 1
        _FROZEN[0] = _FROZEN_IDS[0]
        return self

    def __exit__(self, *exc):
        _FROZEN[0] = self.prev
        return False


def _no_shadow():
    return None


# CWLT_DGRAD_WT_CACHE=0: the per-op layer transposes a weight at every use in the backward instead of once per forward
DGRAD_WT_CACHE = os.environ.get("CWLT_DGRAD_WT_CACHE", "1") != "0"
# CWLT_CAST_MANY=0: refresh the bf16 weight copies with torch's multi-tensor copy instead of cwlt_cast_bf16_many
CAST_MANY = os.environ.get("CWLT_CAST_MANY", "1") != "0"


class ShadowSet:
    """`groups`: tuples of parameters; group i becomes ONE buffer of `dtype` with its members stacked along dim 0
    (a single-member group is a plain cast).  `refresh()` -> list of buffers, up to date with the parameters."""

    def __init__(self, groups, dtype):
        self.dtype = dtype
        self.device = groups[0][0].device
        self.bufs, self.dst, self.src = [], [], []
        for g in groups:
            rows = sum(p.shape[0] for p in g)
            buf = torch.empty((rows,) + tuple(g[0].shape[1:]), dtype=dtype, device=self.device)
            o = 0
            for p in g:
                self.dst.append(buf[o:o + p.shape[0]])
                self.src.append(p)
                o += p.shape[0]
            self.bufs.append(buf)
        self.fresh_in = -1           # id of the frozen_weights scope the buffers were last refreshed in
        self._fast = None            # (parameter addresses, device table or None): the one-launch cast, see _cast_table

    def _cast_table(self):
        """bf16 copies of dense f32 GPU parameters: (table, source base, destination base, n) for cwlt_cast_bf16_many --
        one launch where torch's multi-tensor copy takes four for the 84 tensors of an encoder -- or None (other dtypes,
        or parameters that moved while a capture is running: the multi-tensor copy then).  Rebuilt when a parameter's
        storage moves."""
        ptrs = tuple(p.data_ptr() for p in self.src)
        if self._fast is None or self._fast[0] != ptrs:
            ok = (self.dtype == torch.bfloat16 and self.device.type == "cuda"
                  and all(p.dtype == torch.float32 and p.is_contiguous() for p in self.src)
                  and all(d.is_contiguous() for d in self.dst))
            if ok and torch.cuda.is_current_stream_capturing():
                return None                                  # the table is a host-to-device copy: not inside a capture
            entry = None
            if ok:
                sbase = min(ptrs)
                dbase = min(d.data_ptr() for d in self.dst)
                rows = [((p.data_ptr() - sbase) // 4, (d.data_ptr() - dbase) // 2, p.numel())
                        for p, d in zip(self.src, self.dst)]
                entry = (torch.tensor(rows, dtype=torch.int64).to(self.device), sbase, dbase, len(rows))
            self._fast = (ptrs, entry)
        return self._fast[1]

    def matches(self, dtype, device):
        return self.dtype == dtype and self.device == device and all(p.device == device for p in self.src)

    def __reduce__(self):
        # a cache, not state: copy.deepcopy(model) / torch.save(model) get None and rebuild it on first use (a copied
        # set would have its views detached from its buffers)
        return (_no_shadow, ())

    def refresh(self):
        scope = _FROZEN[0]
        if scope and self.fresh_in == scope and not (self.device.type == "cuda"
                                                     and torch.cuda.is_current_stream_capturing()):
            return self.bufs
        fast = self._cast_table() if CAST_MANY else None
        if fast is not None:
            table, sbase, dbase, n = fast
            _call("cwlt_cast_bf16_many", ctypes.c_void_p(sbase), ctypes.c_void_p(dbase), _lib.dev(table), n,
                  _lib.stream_ptr())
        else:
            with torch.no_grad():
                torch._foreach_copy_(self.dst, [p.detach() for p in self.src])
        self.fresh_in = scope if scope else -1
        return self.bufs


# --------------------------------------------------------------------------------------------------
# causal linear attention
# --------------------------------------------------------------------------------------------------
def scan_segments(N, H, L, dtype, ld_ok=True):
    """Segments per stream the scan kernels should use (1 unless N * H is far below the CU count; bf16 only).
    CWLT_SCAN_SEGMENTS=<n> forces a count (tests, A/B runs): clipped to the number of 64-token chunks."""
    if dtype != torch.bfloat16 or not ld_ok or N * L == 0:
        return 1
    forced = os.environ.get("CWLT_SCAN_SEGMENTS")
    if forced:
        nch = (L + 63) // 64
        want = max(1, min(int(forced), nch))
        cps = -(-nch // want)
        return -(-nch // cps)
    return int(_lib.load().cwlt_scan_segments(N, H, L, _lib.dtype_code(dtype)))


def _seg_ws(N, H, P, backward, device):
    if P <= 1:
        return None
    n = int(_lib.load().cwlt_scan_seg_floats(N, H, P, 1 if backward else 0))
    return torch.empty(n, dtype=torch.float32, device=device)


# One-sweep backward of the bf16 scan (cwlt_causal_linear_bwd_sweep); CWLT_SCAN_SWEEP=0 keeps the dkdv + dq pair.
SCAN_SWEEP = os.environ.get("CWLT_SCAN_SWEEP", "1") != "0"


def _scan_fast(dtype, *lds):
    """Whether a scan call takes the bf16 MFMA kernels (the library decides the same way; its own buffers are dense)."""
    return dtype == torch.bfloat16 and all(x % 8 == 0 for x in lds)


def _check_qkv(fn, q, k, v, cu):
    """q, k, v of one shape and dtype, in either form of the scans -> cu, N, L, H, D.  cu None: (N, L, H, D) sequences.
    Else the packed form, songs laid end to end in ONE row buffer (R, H, D) or (1, R, H, D): cu comes back as the
    SeqOffsets of its R rows, N = n_songs, L = None."""
    if k.shape != q.shape or v.shape != q.shape:
        raise ValueError("%s needs q, k, v of one shape %s" % (fn, "(N, L, H, D)" if cu is None else "(R, H, D)"))
    if q.dtype != k.dtype or q.dtype != v.dtype:
        raise TypeError("q, k, v dtypes differ")
    if cu is None:
        return (None,) + tuple(q.shape)
    _lib.dev(q, "q")
    if q.dim() != 3 and (q.dim() != 4 or q.shape[0] != 1):
        raise ValueError("%s: packed songs are one row buffer, (R, H, D) or (1, R, H, D)" % fn)
    R, H, D = q.shape[-3:]
    cu = _seq_offsets(cu, q.device).check_rows(R)
    return cu, cu.n_songs, None, H, D


def cla_fwd(q, k, v, eps=CLA_EPS, final_state=None, cu=None):
    """q, k, v: (N, L, H, 64) views (row-strided ok) -> q, k, v, out (N, L, H, 64) dense, zinv (N, L, H) f32
    [, fin: the scan's final state for `cla_bwd(final_state=fin)`, or None where the one-sweep backward does not apply
    (f32, odd row strides, segmented few-stream launches) or final_state is False -- a sixth element whenever
    final_state is given (True / False) at all].
    cu (SeqOffsets or n_songs + 1 offsets): the packed form (_check_qkv) -- every song is scanned from its own row 0,
    one workgroup per (song, head), never segmented; out and zinv take q's leading dims, fin is per (song, head)."""
    lib = _lib.load()
    cu, N, L, H, D = _check_qkv("causal linear attention", q, k, v, cu)
    q, ldq = _as_rows(q)
    k, ldk = _as_rows(k)
    v, ldv = _as_rows(v)
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    zinv = torch.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    fast = _scan_fast(q.dtype, ldq, ldk, ldv)
    P = scan_segments(N, H, L, q.dtype, fast) if cu is None else 1
    ws = _seg_ws(N, H, P, False, q.device)
    fin = None
    if final_state and SCAN_SWEEP and fast and P == 1 and q.numel() > 0:
        fin = torch.empty(int(lib.cwlt_scan_final_state_floats(N, H)), dtype=torch.float32, device=q.device)
    # the two entry points differ in their name and in how they say where the sequences are
    name, where, seg = (("", (N, H, L, D), (P, _lib.opt(ws))) if cu is None
                        else ("_packed", (_lib.dev(cu.dev), N, H, D), ()))
    _call("cwlt_causal_linear_fwd" + name, _lib.dev(q, "q"), _lib.dev(k, "k"), _lib.dev(v, "v"), _lib.dev(out),
          _lib.dev(zinv), *where, ldq, ldk, ldv, H * D, float(eps), *seg, _lib.opt(fin), _lib.dtype_code(q.dtype),
          _lib.stream_ptr())
    if final_state is not None:
        return q, k, v, out, zinv, fin
    return q, k, v, out, zinv


def cla_bwd(q, k, v, out, zinv, dout, want_colsum=False, final_state=None, cu=None, per_song=False):
    """-> dqkv (N, L, 3, H, 64): dq | dk | dv side by side (= gradient of a fused QKV projection)
    [, dbias (3*H*64) f32 = its column sums, fused into the kernels on the bf16 path].
    final_state: what `cla_fwd(final_state=True)` returned for these q, k, v -- the backward then runs as one sweep.
    cu: the packed form as in `cla_fwd`, same routes; dqkv takes q's leading dims.  per_song (packed, the bf16 kernels'
    fused column sums only): dbias as the kernels wrote it, (3, n_songs, H*64), not summed."""
    cu, N, L, H, D = _check_qkv("causal linear attention", q, k, v, cu)
    if per_song and cu is None:
        raise ValueError("per-song column sums belong to the packed form")
    dout, lddo = _as_rows(dout)
    q, ldq = _as_rows(q)
    k, ldk = _as_rows(k)
    v, ldv = _as_rows(v)
    lead, R = tuple(q.shape[:-2]), q.numel() // (H * D)
    dqkv = torch.empty(lead + (3, H, D), dtype=q.dtype, device=q.device)
    dq, dk, dv = (_lib.dev(dqkv.select(-3, i)) for i in range(3))
    ld = 3 * H * D
    common = (_lib.dev(q), _lib.dev(k), _lib.dev(v), _lib.dev(out), _lib.dev(zinv), _lib.dev(dout, "dout"))
    code, st = _lib.dtype_code(q.dtype), _lib.stream_ptr()
    name, where = ("", (N, H, L, D)) if cu is None else ("_packed", (_lib.dev(cu.dev), N, H, D))
    fast = _scan_fast(q.dtype, ldq, ldk, ldv, lddo)
    fused = want_colsum and fast
    if final_state is not None and not fast:
        # dout arrived as a view whose row stride the bf16 kernels cannot take (a legal autograd input of the public
        # causal_linear_attention): the final state is simply not used -- the dkdv + dq pair below handles any stride
        final_state = None
    if final_state is not None:
        P, cs = 1, torch.empty((3, N, H * D), dtype=torch.float32, device=q.device) if want_colsum else None
        _call("cwlt_causal_linear_bwd_sweep" + name, *common, _lib.dev(final_state), dq, dk, dv,
              *([_lib.dev(cs[i]) for i in range(3)] if want_colsum else [None] * 3),
              *where, ldq, ldk, ldv, H * D, lddo, ld, ld, ld, code, st)
    else:
        if per_song and not fused:
            raise ValueError("per-song column sums come from the bf16 kernels (row strides % 8 == 0) only")
        P = scan_segments(N, H, L, q.dtype, fast) if cu is None else 1
        ws = _seg_ws(N, H, P, True, q.device)          # shared by the two calls: dkdv fills it, dq reads it
        seg = (P, _lib.opt(ws)) if cu is None else ()
        cs = torch.empty((3, N * P, H * D), dtype=torch.float32, device=q.device) if fused else None
        # dden = -(dout . out) * zinv: written by the reverse scan, read by the dq scan instead of the whole `out` stream
        dden = torch.empty(lead + (H,), dtype=torch.float32, device=q.device) if fast else None
        _call("cwlt_causal_linear_bwd_dkdv" + name, *common, dk, dv, _lib.dev(cs[1]) if fused else None,
              _lib.dev(cs[2]) if fused else None, _lib.opt(dden), *where, ldq, ldk, ldv, H * D, lddo, ld, ld, *seg,
              code, st)
        _call("cwlt_causal_linear_bwd_dq" + name, *common, dq, _lib.dev(cs[0]) if fused else None, _lib.opt(dden),
              *where, ldq, ldk, ldv, H * D, lddo, ld, *seg, code, st)
    if not want_colsum:
        return dqkv
    if cs is None:
        return dqkv, colsum(dqkv.view(R, 3 * H * D))
    if per_song:
        return dqkv, cs
    return dqkv, (cs.sum(1).reshape(3 * H * D) if N * P > 1 else cs.reshape(3 * H * D))


class CausalLinearAttentionFn(torch.autograd.Function):
    """out = CLA(q, k, v): q, k, v (N, L, H, 64) raw projections, elu+1 applied inside the kernel; with cu (a
    SeqOffsets), packed songs as in `cla_fwd`.

    Replaces fast_transformers CausalLinearAttention.forward + causal_dot_product
    (reference call sites: dqn_policy/model.py:128-137,231-232).
    """

    @staticmethod
    def forward(ctx, q, k, v, eps=CLA_EPS, grad_mode=True, cu=None):
        # grad_mode = torch.is_grad_enabled() at the call site (inside forward() it is off; see encoder._EncoderLayerFn)
        q, k, v, out, zinv, fin = cla_fwd(q, k, v, eps, final_state=bool(grad_mode) and any(ctx.needs_input_grad), cu=cu)
        ctx.save_for_backward(q, k, v, out, zinv)
        ctx.fin, ctx.cu = fin, cu
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, zinv = ctx.saved_tensors
        dqkv = cla_bwd(q, k, v, out, zinv, dout, final_state=ctx.fin, cu=ctx.cu)
        return dqkv.select(-3, 0), dqkv.select(-3, 1), dqkv.select(-3, 2), None, None, None


def causal_linear_attention(q, k, v, eps=CLA_EPS, cu=None):
    if cu is not None:
        _lib.dev(q, "q")
        cu = _seq_offsets(cu, q.device)      # built once: forward and backward both read it
    return CausalLinearAttentionFn.apply(q, k, v, eps, torch.is_grad_enabled(), cu)


# ---- packed form: songs of different lengths end to end in one (R, H, 64) row buffer --------------------------------
class SeqOffsets:
    """Row offsets of packed songs: `dev` (n_songs + 1) int32 on the GPU for the kernels, `host` the same numbers as a
    tuple for every check (the kernels trust the table).  Song s owns rows [host[s], host[s + 1])."""

    def __init__(self, cu, device=None, host=None):
        if host is None:
            host = cu.tolist() if torch.is_tensor(cu) else list(cu)
        self.host = tuple(int(x) for x in host)
        h = self.host
        if len(h) < 2 or h[0] != 0:
            raise ValueError("cu_seqlens must hold n_songs + 1 >= 2 row offsets starting at 0")
        if any(b <= a for a, b in zip(h, h[1:])):
            raise ValueError("cu_seqlens must be strictly increasing: an empty song has no rows to scan")
        if h[-1] >= 2 ** 31:
            raise ValueError("packed row offsets are int32")
        if torch.is_tensor(cu) and cu.is_cuda and cu.dtype == torch.int32 and cu.is_contiguous():
            if tuple(cu.shape) != (len(h),):
                raise ValueError("device cu_seqlens and its host copy differ in length")
            self.dev = cu
        else:
            if device is None:
                raise RuntimeError("cu_seqlens must be an int32 GPU tensor (or name the device to put it on)")
            self.dev = torch.tensor(h, dtype=torch.int32, device=device)
        self.n_songs = len(h) - 1
        self.rows = h[-1]
        self.max_len = max(b - a for a, b in zip(h, h[1:]))

    def positions(self):
        """(rows) int32 on the offsets' device: the position of every packed row inside its song (built once)."""
        if getattr(self, "_pos", None) is None:
            h = self.host
            self._pos = torch.cat([torch.arange(b - a, dtype=torch.int32) for a, b in zip(h, h[1:])]).to(self.dev.device)
        return self._pos

    def check_rows(self, rows):
        if rows != self.rows:
            raise ValueError("cu_seqlens ends at row %d, the packed buffer has %d rows" % (self.rows, rows))
        return self


def _seq_offsets(cu, device):
    return cu if isinstance(cu, SeqOffsets) else SeqOffsets(cu, device=device)


def cla_fwd_packed(q, k, v, cu, eps=CLA_EPS, final_state=None):
    """`cla_fwd(cu=cu)`: q, k, v (R, H, 64) -> q, k, v, out (R, H, 64) dense, zinv (R, H) f32 [, fin]."""
    return cla_fwd(q, k, v, eps, final_state, cu=cu)


def cla_bwd_packed(q, k, v, out, zinv, dout, cu, want_colsum=False, final_state=None, per_song=False):
    """`cla_bwd(cu=cu)` -> dqkv (R, 3, H, 64) [, dbias (3*H*64) f32, or (3, n_songs, H*64) with per_song]."""
    return cla_bwd(q, k, v, out, zinv, dout, want_colsum, final_state, cu=cu, per_song=per_song)


def causal_linear_attention_packed(q, k, v, cu, eps=CLA_EPS):
    """Causal linear attention within each song of a packed (R, H, 64) buffer; cu: SeqOffsets or n_songs + 1 offsets."""
    return causal_linear_attention(q, k, v, eps, cu=cu)


# --------------------------------------------------------------------------------------------------
# residual + dropout + LayerNorm
# --------------------------------------------------------------------------------------------------
def ln_fwd(x, a, gamma, beta, eps=LN_EPS, p=0.0, seed=0, save_s=True):
    """s = x + dropout(a); y = LN(s).  x may be None.  a: (rows, D) dense.  -> s (or None), y, mean, rstd."""
    lib = _lib.load()
    rows, D = a.shape
    a = a.contiguous()
    if x is not None:
        x = x.contiguous()
    y = torch.empty_like(a)
    need_s = save_s and (x is not None or p > 0)
    s = torch.empty_like(a) if need_s else None
    mean = torch.empty(rows, dtype=torch.float32, device=a.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=a.device)
    _call("cwlt_add_dropout_layernorm_fwd", _lib.opt(x), _lib.dev(a, "a"), _lib.dev(gamma), _lib.dev(beta), _lib.opt(s), _lib.dev(y),
        _lib.dev(mean), _lib.dev(rstd), rows, D, float(eps), float(p), int(seed), _seed_base(),
        _lib.dtype_code(a.dtype), _lib.stream_ptr())
    if save_s and s is None:
        s = a
    return s, y, mean, rstd


def ln_bwd(dy, dy2, s, gamma, mean, rstd, p=0.0, seed=0, want_dbias=True):
    """-> ds, da, dgamma, dbeta, dbias.  da is ds itself when p == 0."""
    lib = _lib.load()
    rows, D = s.shape
    dy = dy.contiguous()
    if dy2 is not None:
        dy2 = dy2.contiguous()
    ds = torch.empty_like(s)
    da = torch.empty_like(s) if p > 0 else ds
    nb = lib.cwlt_ln_blocks(rows)
    part = torch.empty(nb * 3 * D, dtype=torch.float32, device=s.device)
    stats = torch.empty((3, D), dtype=torch.float32, device=s.device)
    _call("cwlt_add_dropout_layernorm_bwd", _lib.dev(dy, "dy"), _lib.opt(dy2), _lib.dev(s), _lib.dev(gamma), _lib.dev(mean), _lib.dev(rstd),
        _lib.dev(ds), _lib.dev(da) if p > 0 else None, _lib.dev(part), _lib.dev(stats), rows, D, float(p), int(seed), _seed_base(),
        _lib.dtype_code(s.dtype), _lib.stream_ptr())
    return ds, da, stats[0], stats[1], (stats[2] if want_dbias else None)


class LayerNormFn(torch.autograd.Function):
    """Plain LayerNorm over the last dim through the fused kernel (x == NULL, p == 0)."""

    @staticmethod
    def forward(ctx, a, gamma, beta, eps):
        shape = a.shape
        a2 = a.reshape(-1, shape[-1])
        g, b = _f32(gamma), _f32(beta)
        s, y, mean, rstd = ln_fwd(None, a2, g, b, eps, 0.0, 0, save_s=True)
        ctx.save_for_backward(s, g, mean, rstd)
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        s, g, mean, rstd = ctx.saved_tensors
        ds, _, dg, db, _ = ln_bwd(dy.reshape(s.shape), None, s, g, mean, rstd, 0.0, 0, want_dbias=False)
        return ds.view(dy.shape), dg, db, None


def layer_norm(a, gamma, beta, eps=LN_EPS):
    return LayerNormFn.apply(a, gamma, beta, eps)


# --------------------------------------------------------------------------------------------------
# FFN activation, column sums, positional encoding
# --------------------------------------------------------------------------------------------------
def gelu_fwd(h, bias, p=0.0, seed=0, gd_inplace=False):
    """g = dropout(gelu(h + bias)).  gd_inplace: h is OVERWRITTEN with gd = mask / (1 - p) * gelu'(h + bias), the factor
    the backward multiplies the upstream gradient with (gemm_nt_mul); h itself is gone afterwards."""
    lib = _lib.load()
    rows, F = h.shape
    g = torch.empty_like(h)
    _call("cwlt_bias_gelu_dropout_fwd", _lib.dev(h, "h"), _lib.opt(bias), _lib.dev(g), _lib.dev(h) if gd_inplace else None,
          rows, F, float(p), int(seed), _seed_base(), _lib.dtype_code(h.dtype), _lib.stream_ptr())
    return g


# rows from which the hand-written projection GEMM is used (256-row tiles, one workgroup per CU: a step of a few
# thousand token rows leaves most of the chip idle; those keep the library GEMM)
GEMM_BF16_MIN_ROWS = int(os.environ.get("CWLT_GEMM_BF16_MIN_ROWS", 32768))
GEMM_BF16 = os.environ.get("CWLT_GEMM_BF16", "1") != "0"


def gemm_bf16_supported(a, w, c=None, transposed_w=False):
    """Whether `gemm_bf16(a, w, out=c)` can run.  transposed_w: `w` is a transposed VIEW of a stored weight that the
    caller will make contiguous first (the input-gradient forms): only its shape is looked at."""
    return (GEMM_BF16 and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.dim() == 2 and w.dim() == 2
            and a.is_cuda and a.shape[1] == w.shape[1] and a.shape[1] % 64 == 0 and a.shape[1] >= 128
            and w.shape[0] % 8 == 0 and w.shape[0] <= 8192 and a.shape[0] >= GEMM_BF16_MIN_ROWS
            and a.stride(1) == 1 and a.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0
            and (transposed_w or (w.stride(1) == 1 and w.stride(0) % 8 == 0 and w.data_ptr() % 16 == 0))
            and (c is None or (c.dtype == torch.bfloat16 and c.shape == (a.shape[0], w.shape[0]) and c.stride(1) == 1
                               and c.stride(0) % 8 == 0 and c.data_ptr() % 16 == 0)))


def gemm_bf16(a, w, bias=None, out=None, accumulate=False):
    """out (M, N) [+]= a (M, K) @ w (N, K).T [+ bias]: the projection GEMM (csrc/gemm_bf16.hip).  a, w bf16; bias (N)
    f32 or None; out bf16 (allocated when None; accumulate adds onto its contents)."""
    _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("gemm_bf16: accumulate needs the tensor to add onto")
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    _call("cwlt_gemm_bf16", _lib.dev(a, "a"), _lib.dev(w, "w"), _lib.opt(bias), _lib.dev(out, "out"), M, N, K, a.stride(0),
          w.stride(0), out.stride(0), 1 if accumulate else 0, _lib.stream_ptr(), work=2.0 * M * N * K)
    return out


# one encoder layer per host call (csrc/layer.hip, below): CWLT_LAYER_C=0 keeps the per-op path at every size
LAYER_C = os.environ.get("CWLT_LAYER_C", "1") != "0"
LAYER_C_MAX_ROWS = int(os.environ.get("CWLT_LAYER_C_MAX_ROWS", 8192))
# ... and the whole stack of an encoder per host call (one autograd node); CWLT_LAYER_C_STACK=0: one call per layer
LAYER_C_STACK = os.environ.get("CWLT_LAYER_C_STACK", "1") != "0"
# CWLT_GEMM_SMALL_PER_OP=1 (tests): the per-op encoder layer takes its plain projections from cwlt_gemm_bf16_small instead
# of hipBLASLt whenever its rows are few enough for the one-call layer -- then the two paths run the same kernels
GEMM_SMALL_PER_OP = os.environ.get("CWLT_GEMM_SMALL_PER_OP", "0") == "1"


def gemm_small_per_op(x):
    return GEMM_SMALL_PER_OP and x.dtype == torch.bfloat16 and x.dim() == 2 and 0 < x.shape[0] <= LAYER_C_MAX_ROWS


def gemm_bf16_small(a, w, bias=None, out=None, accumulate=False):
    """`gemm_bf16` for few rows (csrc/gemm_small.hip: 64 x 64 output tiles, operands straight from L2): K % 32 == 0."""
    _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("gemm_bf16_small: accumulate needs the tensor to add onto")
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    _call("cwlt_gemm_bf16_small", _lib.dev(a, "a"), _lib.dev(w, "w"), _lib.opt(bias), _lib.dev(out, "out"), M, N, K,
          a.stride(0), w.stride(0), out.stride(0), 1 if accumulate else 0, _lib.stream_ptr(), work=2.0 * M * N * K)
    return out


def gemm_bf16_small_gelu(x, w, bias, p=0.0, seed=0, want_gd=True):
    """`ffn1_gelu_dropout` on the split-K small tiles (csrc/gemm_small.hip), for passes of a few hundred rows at most:
    g = dropout(gelu(x @ w.T + bias)) [, gd = mask / (1 - p) * gelu'(.)] -- bit for bit what `gemm_bf16_small` followed by
    `gelu_fwd(..., gd_inplace=True)` produce.  K % 128 == 0."""
    _lib.load()
    M, K = x.shape
    N = w.shape[0]
    g = torch.empty((M, N), dtype=x.dtype, device=x.device)
    gd = torch.empty((M, N), dtype=x.dtype, device=x.device) if want_gd else None
    _call("cwlt_gemm_bf16_small_gelu", _lib.dev(x, "x"), _lib.dev(w, "w"), _lib.dev(bias), _lib.dev(g), _lib.opt(gd), M, N, K,
          x.stride(0), w.stride(0), float(p), int(seed), _seed_base(), _lib.stream_ptr(), work=2.0 * M * N * K)
    return g, gd


# --------------------------------------------------------------------------------------------------
# one encoder layer per host call (csrc/layer.hip): steps of a few thousand token rows are bound by the HOST when every
# kernel is its own Python-level call (the reference's RL updates: 30 windows x 50 tokens, ~970 launches)
# --------------------------------------------------------------------------------------------------
_LAYER_PLANS = {}


def layer_plan(N, L, D, F, H, p, want_backward):
    """cwlt_encoder_layer_plan, cached: buffer sizes and gradient offsets of one layer call."""
    key = (N, L, D, F, H, p > 0, bool(want_backward))
    plan = _LAYER_PLANS.get(key)
    if plan is None:
        plan = _lib.EncoderLayerPlan()
        _lib.check(_lib.load().cwlt_encoder_layer_plan(N, L, D, F, H, float(p), 1 if want_backward else 0,
                                                       ctypes.byref(plan)), "cwlt_encoder_layer_plan")
        _LAYER_PLANS[key] = plan
    return plan


class LayerCache:
    """What the one-call layers of ONE encoder share: the transposed bf16 weight copies the input-gradient products
    read (all matrices refreshed by one launch, cwlt_transpose_bf16_many) and a scratch buffer (every layer call of
    an encoder runs on the launch stream, one after the other).  `mats`: the bf16 weight buffers, four per layer."""

    def __init__(self, mats, owner):
        self.owner = owner                       # the ShadowSet the buffers belong to (identity = validity)
        dev = mats[0].device
        self.flat = torch.empty(sum(m.numel() for m in mats), dtype=torch.bfloat16, device=dev)
        self.base = mats[0]
        rows, self.views, o = [], [], 0
        for m in mats:
            if m.dtype != torch.bfloat16 or not m.is_contiguous() or m.dim() != 2:
                raise ValueError("LayerCache: dense 2-d bf16 weight buffers expected")
            rows.append(((m.data_ptr() - self.base.data_ptr()) // 2, o, m.shape[0], m.shape[1]))
            self.views.append(self.flat[o:o + m.numel()].view(m.shape[1], m.shape[0]))
            o += m.numel()
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.n = len(mats)
        self.scratch = None
        self.fresh_in = -1

    def __reduce__(self):
        return (_no_shadow, ())                  # a cache, as ShadowSet: copies of a model rebuild it

    def refresh_transposed(self):
        scope = _FROZEN[0]
        if scope and self.fresh_in == scope and not torch.cuda.is_current_stream_capturing():
            return
        _call("cwlt_transpose_bf16_many", _lib.dev(self.base), _lib.dev(self.flat), _lib.dev(self.table), self.n,
              _lib.stream_ptr())
        self.fresh_in = scope if scope else -1

    def setup_stack(self, layer_params, weights, qkv_bias, dims):
        """Whole-stack calls (encoder._EncoderStackFn): a persistent HOST array of cwlt_encoder_layer structs with
        everything that does not change from call to call filled in once -- dims = (d_model, d_ff, n_heads), the bf16
        weight buffers (four per layer, persistent ShadowSet storage), their transposed copies, the stacked f32 Q/K/V
        biases -- and the flat list of the layers' parameters (16 per layer, encoder._layer_params order)."""
        n = len(qkv_bias)
        arr = (_lib.EncoderLayer * n)()
        D, F, H = dims
        for i in range(n):
            st = arr[i]
            st.d_model, st.d_ff, st.n_heads, st.ln_eps, st.attn_eps = D, F, H, LN_EPS, CLA_EPS
            st.wqkv, st.wo, st.w1, st.w2 = (t.data_ptr() for t in weights[4 * i:4 * i + 4])
            st.wqkv_t, st.wo_t, st.w1_t, st.w2_t = (t.data_ptr() for t in self.views[4 * i:4 * i + 4])
            st.bqkv = qkv_bias[i].data_ptr()
        self.arr = arr
        self.params = list(layer_params)
        self.all_need_grad = all(q.requires_grad for q in self.params)
        self.dims = dims
        self.qkv_bias_owner = qkv_bias
        self._grads = None

    def grad_buffer(self, plan):
        """(grads, views): a persistent f32 buffer for the parameter gradients of one backward of the whole stack and the
        view of each parameter's gradient in it, in the order of self.params."""
        n = len(self.arr)
        gf = plan.grad_floats
        got = self._grads
        if got is None or got[0].numel() != n * gf or torch.cuda.is_current_stream_capturing():
            D, F, _ = self.dims
            grads = torch.empty(n * gf, dtype=torch.float32, device=self.flat.device)
            go = list(plan.grad_off)
            views = []
            for i in range(n):
                def gv(j, *shape):
                    m = 1
                    for d_ in shape:
                        m *= d_
                    return grads[i * gf + go[j]:i * gf + go[j] + m].view(shape)
                wqkv, bqkv = gv(0, 3 * D, D), gv(1, 3 * D)
                # q / k / v weight (bias) gradients are the row blocks of the stacked ones
                views += [wqkv[:D], bqkv[:D], wqkv[D:2 * D], bqkv[D:2 * D], wqkv[2 * D:], bqkv[2 * D:], gv(2, D, D), gv(3, D),
                          gv(4, F, D), gv(5, F), gv(6, D, F), gv(7, D), gv(8, D), gv(9, D), gv(10, D), gv(11, D)]
            got = (grads, views)
            if not torch.cuda.is_current_stream_capturing():
                self._grads = got
        return got

    def get_scratch(self, nbytes):
        dev = self.flat.device
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)     # lives in the graph's pool
        if self.scratch is None or self.scratch.numel() < nbytes:
            self.scratch = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
        return self.scratch


def encoder_fwd(arr, n):
    _call("cwlt_encoder_fwd", arr, n, _lib.stream_ptr())


def encoder_bwd(arr, n):
    _call("cwlt_encoder_bwd", arr, n, _lib.stream_ptr())


def encoder_layer_fwd(st):
    _call("cwlt_encoder_layer_fwd", ctypes.byref(st), _lib.stream_ptr())


def encoder_layer_bwd(st):
    _call("cwlt_encoder_layer_bwd", ctypes.byref(st), _lib.stream_ptr())


def gemm_nt_mul_supported(a, w, g):
    return (a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and a.dim() == 2
            and w.dim() == 2 and g.dim() == 2 and w.shape[0] % 256 == 0 and a.shape[1] % 64 == 0
            and a.shape[1] == w.shape[1] and g.shape == (a.shape[0], w.shape[0])
            and all(t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (a, w, g)))


def gemm_nt_mul(a, w, g, want_colsum=True):
    """c = (a @ w.T) * g in one kernel, + column sums of c.  a (M, K), w (N, K), g (M, N) bf16 -> c (M, N) bf16
    [, colsum (N) f32].  The FFN backward: a = dy, w = linear2.weight.T (contiguous), g = gd."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty((M, N), dtype=a.dtype, device=a.device)
    part = cs = None
    if want_colsum:
        part = torch.empty(lib.cwlt_gemm_nt_tiles(M) * N, dtype=torch.float32, device=a.device)
        cs = torch.empty(N, dtype=torch.float32, device=a.device)
    _call("cwlt_gemm_nt_mul", _lib.dev(a, "a"), _lib.dev(w, "w"), _lib.dev(g, "g"), _lib.dev(c), _lib.opt(part),
          _lib.opt(cs), M, N, K, a.stride(0), w.stride(0), g.stride(0), N, _lib.stream_ptr(), work=2.0 * M * N * K)
    return (c, cs) if want_colsum else c


def ffn1_fused_supported(x, w, bias):
    return (x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and bias.dtype == torch.float32 and x.dim() == 2
            and w.dim() == 2 and w.shape[0] % 256 == 0 and x.shape[1] % 64 == 0 and x.shape[1] == w.shape[1]
            and bias.numel() == w.shape[0] and bias.is_contiguous() and bias.data_ptr() % 16 == 0
            and all(t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (x, w)))


def ffn1_gelu_dropout(x, w, bias, p=0.0, seed=0):
    """g = dropout(gelu(x @ w.T + bias)) and gd = mask / (1 - p) * gelu'(x @ w.T + bias) in ONE kernel (the GEMM's
    epilogue): what `torch.mm` + `gelu_fwd(..., gd_inplace=True)` produce, without the pre-activation's round trip
    through HBM.  x (M, K), w (N, K) bf16, bias (N) f32 -> g, gd (M, N) bf16."""
    _lib.load()
    M, K = x.shape
    N = w.shape[0]
    g = torch.empty((M, N), dtype=x.dtype, device=x.device)
    gd = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _call("cwlt_gemm_nt_bias_gelu_dropout", _lib.dev(x, "x"), _lib.dev(w, "w"), _lib.dev(bias), _lib.dev(g), _lib.dev(gd),
          M, N, K, x.stride(0), w.stride(0), float(p), int(seed), _seed_base(), _lib.stream_ptr(), work=2.0 * M * N * K)
    return g, gd


# rows from which the one-kernel residual block is used (128-row tiles, one workgroup per CU: below ~2 tiles per CU the
# hipBLASLt GEMM + LayerNorm kernel pair fills the chip better)
LINEAR_LN_MIN_ROWS = int(os.environ.get("CWLT_LINEAR_LN_MIN_ROWS", 65536))
# ... and the reduction lengths: at K = 512 (the out-projection) the one-kernel form takes 0.61 ms against 0.36 + 0.44
# for the pair at R = 524 288; at K = 2048 (linear2) its serial epilogue (one workgroup per CU: nothing runs beside
# it) costs more than the pair's extra stream, 1.43 against 0.96 + 0.42 ms (profiles/r03_linear_ln_microbench.txt)
LINEAR_LN_MAX_K = int(os.environ.get("CWLT_LINEAR_LN_MAX_K", 1024))
FUSED_LINEAR_LN = os.environ.get("CWLT_FUSED_LINEAR_LN", "1") != "0"


def linear_ln_supported(a, w, x):
    return (FUSED_LINEAR_LN and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x is not None
            and x.dtype == torch.bfloat16 and a.dim() == 2 and w.dim() == 2 and w.shape[0] == 512
            and a.shape[1] == w.shape[1] and a.shape[1] % 64 == 0 and x.shape == (a.shape[0], 512) and x.is_contiguous()
            and a.shape[0] >= LINEAR_LN_MIN_ROWS and a.shape[1] <= LINEAR_LN_MAX_K
            and all(t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (a, w)))


def linear_ln(a, w, bias, x, gamma, beta, eps=LN_EPS, p=0.0, seed=0):
    """s = x + dropout(a @ w.T + bias); y = LayerNorm(s) in ONE kernel (the GEMM's epilogue): what `torch.addmm` +
    `ln_fwd` produce without the projection's output ever reaching HBM.  a (M, K), w (512, K), x (M, 512) bf16;
    bias, gamma, beta (512) f32 -> s, y (M, 512) bf16, mean, rstd (M) f32."""
    _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if x.shape != (M, N) or not x.is_contiguous() or x.dtype != a.dtype:
        raise ValueError("linear_ln: the residual must be a dense (%d, %d) tensor of the operands' dtype" % (M, N))
    s = torch.empty((M, N), dtype=a.dtype, device=a.device)
    y = torch.empty((M, N), dtype=a.dtype, device=a.device)
    mean = torch.empty(M, dtype=torch.float32, device=a.device)
    rstd = torch.empty(M, dtype=torch.float32, device=a.device)
    _call("cwlt_gemm_nt_bias_dropout_add_layernorm", _lib.dev(a, "a"), _lib.dev(w, "w"), _lib.dev(bias), _lib.dev(x, "x"),
          _lib.dev(gamma), _lib.dev(beta), _lib.dev(s), _lib.dev(y), _lib.dev(mean), _lib.dev(rstd), M, N, K, a.stride(0),
          w.stride(0), float(eps), float(p), int(seed), _seed_base(), _lib.stream_ptr(), work=2.0 * M * N * K)
    return s, y, mean, rstd


def gelu_bwd(dg, h, bias, p=0.0, seed=0, want_dbias=True):
    lib = _lib.load()
    rows, F = h.shape
    dg = dg.contiguous()
    dh = torch.empty_like(h)
    part = dbias = None
    if want_dbias:
        part = torch.empty(lib.cwlt_rowslab_blocks(rows) * F, dtype=torch.float32, device=h.device)
        dbias = torch.empty(F, dtype=torch.float32, device=h.device)
    _call("cwlt_bias_gelu_dropout_bwd", _lib.dev(dg, "dg"), _lib.dev(h), _lib.opt(bias), _lib.dev(dh),
                                              _lib.opt(part), _lib.opt(dbias), rows, F, float(p), int(seed), _seed_base(),
                                              _lib.dtype_code(h.dtype), _lib.stream_ptr())
    return dh, dbias


def wgrad_supported(a, b):
    return (a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.dim() == 2 and b.dim() == 2
            and a.shape[1] % 8 == 0 and b.shape[1] % 8 == 0 and a.stride(1) == 1 and b.stride(1) == 1
            and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def wgrad(a, b, out=None, accumulate=False):
    """out (N1, N2) f32 (+)= a^T b;  a (M, N1), b (M, N2) bf16 row-major.  The weight gradient of a Linear with
    input b and output gradient a.  `out` may be a dense f32 .grad view (written in place)."""
    lib = _lib.load()
    M, N1 = a.shape
    N2 = b.shape[1]
    S = lib.cwlt_wgrad_splits(M, N1, N2)
    part = torch.empty(S * N1 * N2, dtype=torch.float32, device=a.device)
    if out is None:
        out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
        accumulate = False
    _call("cwlt_wgrad_bf16", _lib.dev(a, "a"), _lib.dev(b, "b"), _lib.dev(part), _lib.dev(out), M, N1, N2,
          a.stride(0), b.stride(0), 1 if accumulate else 0, _lib.stream_ptr(), work=2.0 * M * N1 * N2)
    return out


def wgrad_group(pairs, accumulate=False, outs=None):
    """[(a_i, b_i)] (at most four, all with the same number of rows, widths multiples of 256) -> [a_i^T b_i] f32, as ONE
    launch + one reduce launch (cwlt_wgrad_bf16_group): bit-identical to `wgrad` on every pair."""
    lib = _lib.load()
    n = len(pairs)
    M = pairs[0][0].shape[0]
    parts, res = [], []
    for i, (a, b) in enumerate(pairs):
        N1, N2 = a.shape[1], b.shape[1]
        parts.append(torch.empty(lib.cwlt_wgrad_splits(M, N1, N2) * N1 * N2, dtype=torch.float32, device=a.device))
        res.append(outs[i] if outs is not None else torch.empty((N1, N2), dtype=torch.float32, device=a.device))
    vp = ctypes.c_void_p * n
    _call("cwlt_wgrad_bf16_group", vp(*[a.data_ptr() for a, _ in pairs]), vp(*[b.data_ptr() for _, b in pairs]),
          vp(*[t.data_ptr() for t in parts]), vp(*[t.data_ptr() for t in res]),
          (ctypes.c_int * n)(*[a.shape[1] for a, _ in pairs]), (ctypes.c_int * n)(*[b.shape[1] for _, b in pairs]),
          (ctypes.c_int64 * n)(*[a.stride(0) for a, _ in pairs]), (ctypes.c_int64 * n)(*[b.stride(0) for _, b in pairs]),
          n, M, 1 if accumulate else 0, _lib.stream_ptr())
    return res


class LinearWgradFn(torch.autograd.Function):
    """y = x @ w.T + b for a bf16 activation x and f32 master parameters (in_linear, the fused head projection).
    Same forward as F.linear on the bf16 casts; the backward takes the weight gradient with the split-K MFMA kernel
    straight in f32 (no bf16 rounding of the gradient, no .float() pass) and the bias gradient with the
    deterministic column sum."""

    @staticmethod
    def forward(ctx, x, w, b):
        w16, b16 = _cast_pair(w, b, x.dtype)
        ctx.save_for_backward(x)
        ctx.w16 = w16              # a persistent shadow buffer when w is a Parameter: not version-tracked on purpose
        if gemm_bf16_supported(x, w16):
            return gemm_bf16(x, w16, _f32(b))
        return torch.addmm(b16, x, w16.t())

    @staticmethod
    def backward(ctx, dy):
        (x,), w16 = ctx.saved_tensors, ctx.w16
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = (gemm_bf16(dy, w16.t().contiguous()) if gemm_bf16_supported(dy, w16.t(), transposed_w=True)
                  else torch.mm(dy, w16))
        dw = wgrad(dy, x) if wgrad_supported(dy, x) else torch.mm(dy.t(), x).float()
        return dx, dw, colsum(dy)


def _cast_pair(w, b, dtype):
    """(w, b) in `dtype`; for a Parameter pair through a ShadowSet kept on the weight (no per-call cast kernels)."""
    if w.dtype == dtype and b.dtype == dtype:
        return w, b
    if isinstance(w, torch.nn.Parameter) and isinstance(b, torch.nn.Parameter):
        sh = getattr(w, "_cwlt_shadow", None)
        if sh is None or not sh.matches(dtype, w.device) or sh.src[1] is not b:
            sh = w._cwlt_shadow = ShadowSet([(w,), (b,)], dtype)
        w16, b16 = sh.refresh()
        return w16, b16
    return w.to(dtype), b.to(dtype)


def linear(x, w, b):
    """F.linear(x, w.to(x.dtype), b.to(x.dtype)) with the f32-gradient backward above when x is bf16."""
    if x.dtype == torch.bfloat16 and x.dim() == 2 and x.is_contiguous() and torch.is_grad_enabled():
        return LinearWgradFn.apply(x, w, b)
    if not torch.is_grad_enabled():
        w16, b16 = _cast_pair(w, b, x.dtype)
        if x.dim() == 2 and gemm_bf16_supported(x, w16):
            return gemm_bf16(x, w16, _f32(b))
        return torch.nn.functional.linear(x, w16, b16)
    return torch.nn.functional.linear(x, w.to(x.dtype), b.to(x.dtype))


def colsum(x):
    """Deterministic column sums of a (rows, ncols) matrix (row-strided ok) -> (ncols) f32."""
    lib = _lib.load()
    rows, ncols = x.shape
    if x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0 or ncols % 8 != 0:
        return x.float().sum(0)
    part = torch.empty(lib.cwlt_colsum_blocks(rows) * ncols, dtype=torch.float32, device=x.device)
    out = torch.empty(ncols, dtype=torch.float32, device=x.device)
    _call("cwlt_colsum", _lib.dev(x, "x"), _lib.dev(part), _lib.dev(out), rows, ncols, x.stride(0),
                               _lib.dtype_code(x.dtype), _lib.stream_ptr())
    return out


def _check_pos(pos, rows, T, pe):
    """pos: (rows) int32 on the GPU, positions of packed rows; T: the longest song (a host number: the kernels trust the
    table, so what is checked is that the caller's bound fits the positional buffer)."""
    if pe is None:
        raise ValueError("pos= needs the positional table")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (rows,) or not pos.is_contiguous():
        raise ValueError("pos must be a dense int32 tensor with one entry per row")
    if int(T) < 1 or int(T) > pe.shape[0]:
        raise RuntimeError("longest song %d exceeds the positional table (%d)" % (int(T), pe.shape[0]))


def posenc_dropout(x, pe, T, p=0.0, seed=0, pos=None):
    """x (rows, D) dense; pe (max_len, D) f32 or None -> dropout(x + pe[r % T]).
    pos (rows) int32, optional: dropout(x + pe[pos[r]]) for packed songs, T then the longest song (every pos < T); the
    dropout stream of row r is the same either way."""
    lib = _lib.load()
    rows, D = x.shape
    x = x.contiguous()
    y = torch.empty_like(x)
    if pos is not None:
        _check_pos(pos, rows, T, pe)
        _call("cwlt_posenc_dropout_pos", _lib.dev(x, "x"), _lib.dev(pe), _lib.dev(pos, "pos"), _lib.dev(y), rows, D,
              float(p), int(seed), _seed_base(), _lib.dtype_code(x.dtype), _lib.stream_ptr())
        return y
    _call("cwlt_posenc_dropout", _lib.dev(x, "x"), _lib.opt(pe), _lib.dev(y), rows, int(T), D, float(p),
                                       int(seed), _seed_base(), _lib.dtype_code(x.dtype), _lib.stream_ptr())
    return y


class PosEncDropoutFn(torch.autograd.Function):
    """PositionalEncoding.forward (dqn_policy/model.py:90-92): dropout(x + pe[:, :T])."""

    @staticmethod
    def forward(ctx, x, pe, p, seed):
        N, T, D = x.shape
        if pe is not None and T > pe.shape[-2]:
            raise RuntimeError("sequence length %d exceeds the positional table (%d)" % (T, pe.shape[-2]))
        ctx.p, ctx.seed, ctx.T = p, seed, T
        return posenc_dropout(x.reshape(N * T, D), None if pe is None else pe.reshape(-1, D), T, p,
                              seed).view(N, T, D)

    @staticmethod
    def backward(ctx, dy):
        if ctx.p == 0:
            return dy, None, None, None
        N, T, D = dy.shape
        return posenc_dropout(dy.reshape(N * T, D), None, T, ctx.p, ctx.seed).view(N, T, D), None, None, None


class PosEncDropoutPosFn(torch.autograd.Function):
    """PosEncDropoutFn for packed songs: x (R, D), row r at position pos[r] (int32 on the GPU), max_len the longest
    song.  The backward never reads pe, so it is the rectangular one."""

    @staticmethod
    def forward(ctx, x, pe, pos, max_len, p, seed):
        R, D = x.shape
        ctx.p, ctx.seed, ctx.T = p, seed, int(max_len)
        return posenc_dropout(x, pe.reshape(-1, D), max_len, p, seed, pos=pos)

    @staticmethod
    def backward(ctx, dy):
        if ctx.p == 0:
            return dy, None, None, None, None, None
        return posenc_dropout(dy, None, ctx.T, ctx.p, ctx.seed), None, None, None, None, None


# --------------------------------------------------------------------------------------------------
# compound-word embedding
# --------------------------------------------------------------------------------------------------
class CWEmbedFn(torch.autograd.Function):
    """tokens (..., A) int64 + A tables -> (..., sum widths): lut_f(x_f) * sqrt(d_f), concatenated."""

    @staticmethod
    def forward(ctx, tokens, out_dtype, *tables):
        lib = _lib.load()
        A = len(tables)
        if tokens.shape[-1] != A:
            raise ValueError("tokens carry %d attributes, model has %d tables" % (tokens.shape[-1], A))
        if tokens.dtype != torch.int64:
            raise TypeError("tokens must be int64 (the reference indexes nn.Embedding with .long())")
        tabs = [_f32(t) for t in tables]
        widths = [t.shape[1] for t in tabs]
        nrows = [t.shape[0] for t in tabs]
        tok = tokens.reshape(-1, A).contiguous()
        rows = tok.shape[0]
        dcat = sum(widths)
        out = torch.empty((rows, dcat), dtype=out_dtype, device=tok.device)
        _call("cwlt_cw_embed_fwd", _lib.dev(tok, "tokens"), _lib.ptr_array(tabs), _lib.int_array(widths),
                                         _lib.int_array(nrows), A, _lib.dev(out), rows, dcat,
                                         _lib.dtype_code(out_dtype), _lib.stream_ptr())
        ctx.save_for_backward(tok)
        ctx.widths, ctx.nrows = widths, nrows
        return out.view(*tokens.shape[:-1], dcat)

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (tok,) = ctx.saved_tensors
        widths, nrows = ctx.widths, ctx.nrows
        A = len(widths)
        dcat = sum(widths)
        d2 = dout.reshape(-1, dcat).contiguous()
        rows = d2.shape[0]
        total = sum(w * n for w, n in zip(widths, nrows))
        part = torch.empty(lib.cwlt_embed_splits(rows) * total, dtype=torch.float32, device=d2.device)
        flat = torch.empty(total, dtype=torch.float32, device=d2.device)
        _call("cwlt_cw_embed_bwd", _lib.dev(tok), _lib.int_array(widths), _lib.int_array(nrows), A,
                                         _lib.dev(d2, "dout"), _lib.dev(part), _lib.dev(flat), rows, dcat,
                                         _lib.dtype_code(d2.dtype), _lib.stream_ptr())
        grads, o = [], 0
        for w, n in zip(widths, nrows):
            grads.append(flat[o:o + w * n].view(n, w))
            o += w * n
        return (None, None) + tuple(grads)


def cw_embed(tokens, tables, out_dtype=torch.float32):
    return CWEmbedFn.apply(tokens, out_dtype, *tables)


EMBED_PROJ = os.environ.get("CWLT_EMBED_PROJ", "1") != "0"
# below this many token rows the front's three kernels cost nothing on the GPU and the ~14 small launches that build the
# projected tables are a net loss for the launch-bound RL steps
EMBED_PROJ_MIN_ROWS = int(os.environ.get("CWLT_EMBED_PROJ_MIN_ROWS", "8192"))


class EmbedProjFn(torch.autograd.Function):
    """The model's input front in one pass (dqn_policy/model.py:206-223 + 90-92):
    dropout(in_linear(cat_f(lut_f(x_f) * sqrt(d_f))) + pe[:, :T]) = dropout(sum_f P_f[x_f] + b + pe) with the projected
    tables P = cat_f(sqrt(d_f) lut_f . W_in[:, cols_f]^T) ((sum n_f, D) f32, built by the caller with differentiable
    torch ops, so autograd carries dP on to the tables and to in_linear.weight).  tokens (N, T, A) int64 ->
    (N, T, D) of `out_dtype`.  Backward: dP = the scatter-add of the gradient in front of the dropout over the ids (the
    one-hot MFMA GEMM of cwlt_cw_embed_bwd), db = the column sum of one attribute's rows of dP."""

    @staticmethod
    def forward(ctx, tokens, tproj, bias, pe, nrows, p, seed, out_dtype, pos=None, max_len=None):
        if tokens.dtype != torch.int64:
            raise TypeError("tokens must be int64 (the reference indexes nn.Embedding with .long())")
        N, T, A = tokens.shape
        if A != len(nrows):
            raise ValueError("tokens carry %d attributes, model has %d tables" % (A, len(nrows)))
        D = tproj.shape[1]
        if tproj.shape[0] != sum(nrows) or bias.shape != (D,):
            raise ValueError("projected tables / bias do not match the vocabularies")
        if pe is not None:
            pe = pe.reshape(-1, D)
            if pos is None and T > pe.shape[0]:
                raise RuntimeError("sequence length %d exceeds the positional table (%d)" % (T, pe.shape[0]))
        tok = tokens.reshape(-1, A).contiguous()
        rows = tok.shape[0]
        tp = tproj.detach().to(out_dtype).contiguous()
        out = torch.empty((rows, D), dtype=out_dtype, device=tok.device)
        if pos is not None:
            _check_pos(pos, rows, max_len, pe)
            _call("cwlt_cw_embed_proj_fwd_pos", _lib.dev(tok, "tokens"), _lib.dev(tp), _lib.int_array(nrows), A,
                  _lib.dev(_f32(bias)), _lib.dev(_f32(pe)), _lib.dev(pos, "pos"), _lib.dev(out), rows, D, float(p),
                  int(seed), _seed_base(), _lib.dtype_code(out_dtype), _lib.stream_ptr())
        else:
            _call("cwlt_cw_embed_proj_fwd", _lib.dev(tok, "tokens"), _lib.dev(tp), _lib.int_array(nrows), A,
                  _lib.dev(_f32(bias)), _lib.opt(None if pe is None else _f32(pe)), _lib.dev(out), rows, int(T), D,
                  float(p), int(seed), _seed_base(), _lib.dtype_code(out_dtype), _lib.stream_ptr())
        ctx.save_for_backward(tok)
        ctx.cfg = (list(nrows), T, D, p, seed)
        ctx.pos_form = pos is not None
        return out.view(N, T, D)

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (tok,) = ctx.saved_tensors
        nrows, T, D, p, seed = ctx.cfg
        A = len(nrows)
        d2 = dout.reshape(-1, D)
        dpre = posenc_dropout(d2, None, T, p, seed) if p > 0 else d2.contiguous()
        rows = dpre.shape[0]
        total = sum(nrows) * D
        part = torch.empty(lib.cwlt_embed_splits(rows) * total, dtype=torch.float32, device=dpre.device)
        dtp = torch.empty((sum(nrows), D), dtype=torch.float32, device=dpre.device)
        _call("cwlt_cw_embed_proj_bwd", _lib.dev(tok), _lib.int_array(nrows), A, D, _lib.dev(dpre, "dpre"), _lib.dev(part),
              _lib.dev(dtp), rows, D, _lib.dtype_code(dpre.dtype), _lib.stream_ptr())
        dbias = dtp[:nrows[0]].sum(0)             # every token row has exactly one id of attribute 0
        return (None, dtp, dbias) + (None,) * (5 if ctx.pos_form is False else 7)


def embed_proj(tokens, tables, w_in, b_in, pe, p, seed, out_dtype, pos=None, max_len=None):
    """tokens (N, T, A); tables: A embedding weights (n_f, d_f) f32; w_in (D, sum d_f), b_in (D); pe (.., max_len, D).
    pos (N * T) int32 with max_len = the longest song: packed songs, row r at position pos[r] in place of r % T."""
    cols, parts = 0, []
    for t in tables:
        d = t.shape[1]
        parts.append(torch.nn.functional.linear(t * math.sqrt(d), w_in[:, cols:cols + d]))
        cols += d
    tproj = torch.cat(parts, 0)
    if pos is None:
        return EmbedProjFn.apply(tokens, tproj, b_in, pe, tuple(t.shape[0] for t in tables), p, seed, out_dtype)
    return EmbedProjFn.apply(tokens, tproj, b_in, pe, tuple(t.shape[0] for t in tables), p, seed, out_dtype, pos, max_len)


# --------------------------------------------------------------------------------------------------
# per-attribute heads
# --------------------------------------------------------------------------------------------------
def heads_forward(logits, n_class, target=None, mask=None, want_argmax=False, want_pmax=False, want_probs=False):
    """logits (rows, ld).  -> dict(loss_sum (A) f32 | argmax (rows, A) | pmax | probs (rows, sum n))."""
    lib = _lib.load()
    rows, ld = logits.shape[0], logits.stride(0)
    A = len(n_class)
    dev = logits.device
    res = {}
    loss_part = loss_sum = None
    if target is not None:
        target = target.reshape(rows, A).contiguous()
        loss_part = torch.empty(lib.cwlt_heads_blocks(rows) * A, dtype=torch.float32, device=dev)
        loss_sum = res["loss_sum"] = torch.empty(A, dtype=torch.float32, device=dev)
    if mask is not None:
        mask = mask.reshape(rows).float().contiguous()
    am = res["argmax"] = torch.empty((rows, A), dtype=torch.int64, device=dev) if want_argmax else None
    pm = res["pmax"] = torch.empty((rows, A), dtype=torch.float32, device=dev) if want_pmax else None
    ncol = sum(n_class)
    pr = res["probs"] = torch.empty((rows, ncol), dtype=torch.float32, device=dev) if want_probs else None
    _call("cwlt_heads_fwd", _lib.dev(logits, "logits"), _lib.int_array(n_class), A, _lib.opt(target),
                                  _lib.opt(mask), _lib.opt(loss_part), _lib.opt(loss_sum), _lib.opt(am),
                                  _lib.opt(pm), _lib.opt(pr), rows, ld, ncol, _lib.dtype_code(logits.dtype),
                                  _lib.stream_ptr())
    return res


def heads_tiled(logits, n_class, dlogits=None):
    """True when heads_forward / heads_ce / logp_argmax run `logits` (and the gradient buffer `dlogits` of a backward)
    on the tiled kernels, False on the wave-per-row kernels: the launchers' own decision (cwlt_heads_tiled)."""
    st = _lib.load().cwlt_heads_tiled(_lib.int_array(n_class), len(n_class), logits.stride(0),
                                      _lib.dtype_code(logits.dtype), _lib.dev(logits, "logits"), _lib.opt(dlogits))
    if st < 0:
        _lib.check(-st, "cwlt_heads_tiled")
    return st == 1


class HeadsCEFn(torch.autograd.Function):
    """6 x compute_loss (dqn_policy/model.py:163-197): returns the (A) vector of masked-mean CE losses."""

    @staticmethod
    def forward(ctx, logits, target, mask, n_class):
        logits = logits.contiguous()   # dense (rows, W >= sum n_class): the bwd kernel zero-fills cols up to W
        rows = logits.shape[0]
        mask_f = mask.reshape(rows).float().contiguous()
        target = target.reshape(rows, len(n_class)).contiguous()
        res = heads_forward(logits, n_class, target, mask_f)
        msum = mask_f.sum()
        ctx.save_for_backward(logits, target, mask_f, msum)
        ctx.n_class = n_class
        return res["loss_sum"] / msum

    @staticmethod
    def backward(ctx, gloss):
        lib = _lib.load()
        logits, target, mask_f, msum = ctx.saved_tensors
        n_class = ctx.n_class
        coef = (gloss.float() / msum).contiguous()
        dlogits = torch.empty_like(logits)
        _call("cwlt_heads_ce_bwd", _lib.dev(logits), _lib.int_array(n_class), len(n_class), _lib.dev(target),
                                         _lib.dev(mask_f), _lib.dev(coef), _lib.dev(dlogits), logits.shape[0],
                                         logits.stride(0), _lib.dtype_code(logits.dtype), _lib.stream_ptr())
        return dlogits, None, None, None


def heads_ce(logits, target, mask, n_class):
    """logits (rows, >= sum n_class) dense rows; -> (A) losses = sum(mask * nll) / sum(mask) per attribute."""
    return HeadsCEFn.apply(logits, target, mask, tuple(int(n) for n in n_class))


# --------------------------------------------------------------------------------------------------
# banded attention (AIRL discriminator)
# --------------------------------------------------------------------------------------------------
def band_attention(q, k, v, mask, window, p=0.0, seed=0, want_lse=False):
    """q, k, v: (B, L, H, 64) views; mask (B, L) nonzero = attend or None; window = one-sided width.
    -> (B, L, H*64)  [, lse (B, H, L) f32 when want_lse]."""
    B, L, H, D = q.shape
    q, ldq = _as_rows(q)
    k, ldk = _as_rows(k)
    v, ldv = _as_rows(v)
    out = torch.empty((B, L, H * D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device) if want_lse else None
    if mask is not None:
        mask = mask.reshape(B, L).float().contiguous()
    _call("cwlt_band_attn_fwd", _lib.dev(q, "q"), _lib.dev(k, "k"), _lib.dev(v, "v"), _lib.opt(mask), _lib.dev(out),
          _lib.opt(lse), B, H, L, D, int(window), ldq, ldk, ldv, H * D, 1.0 / math.sqrt(D), float(p), int(seed), _seed_base(),
          _lib.dtype_code(q.dtype), _lib.stream_ptr())
    return (out, lse) if want_lse else out


class BandAttentionFn(torch.autograd.Function):
    """Band attention over one fused projection buffer qkv (B, L, 3, H, 64) -> (B, L, H*64); the backward
    writes the three gradients straight into the column blocks of one (B, L, 3, H, 64) buffer."""

    @staticmethod
    def forward(ctx, qkv, mask, window, p, seed):
        qkv = qkv.contiguous()
        B, L, _, H, D = qkv.shape
        if mask is not None:
            mask = mask.reshape(B, L).float().contiguous()
        out, lse = band_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, window, p, seed, want_lse=True)
        ctx.save_for_backward(qkv, out, lse, mask)
        ctx.cfg = (int(window), float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask = ctx.saved_tensors
        window, p, seed = ctx.cfg
        B, L, _, H, D = qkv.shape
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        ld = 3 * H * D
        views = [_as_rows(t[:, :, i])[0] for t in (qkv, dqkv) for i in range(3)]
        q, k, v, dq, dk, dv = views
        if any(t.data_ptr() != src[:, :, i].data_ptr() for src, ts in ((qkv, views[:3]), (dqkv, views[3:]))
               for i, t in enumerate(ts)):
            raise RuntimeError("band attention backward needs the fused (B, L, 3, H, 64) layout")
        _call("cwlt_band_attn_bwd", _lib.dev(q, "q"), _lib.dev(k, "k"), _lib.dev(v, "v"), _lib.opt(mask),
              _lib.dev(out), _lib.dev(lse), _lib.dev(dout, "dout"), _lib.dev(dq, "dq"), _lib.dev(dk, "dk"),
              _lib.dev(dv, "dv"), B, H, L, D, window, ld, ld, ld, H * D, H * D, ld, ld, ld, 1.0 / math.sqrt(D), p, seed, _seed_base(),
              _lib.dtype_code(qkv.dtype), _lib.stream_ptr())
        return dqkv, None, None, None, None


class AddDropoutLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + dropout(a)) (x may be None) -- the post-LN residual block of BertSelfOutput /
    LongformerOutput, differentiable.  gamma / beta f32."""

    @staticmethod
    def forward(ctx, x, a, gamma, beta, eps, p, seed):
        g, b = _f32(gamma), _f32(beta)
        s, y, mean, rstd = ln_fwd(x, a, g, b, eps, p, seed, save_s=True)
        ctx.save_for_backward(s, g, mean, rstd)
        ctx.cfg = (x is not None, float(p), int(seed))
        return y

    @staticmethod
    def backward(ctx, dy):
        s, g, mean, rstd = ctx.saved_tensors
        has_x, p, seed = ctx.cfg
        ds, da, dg, db, _ = ln_bwd(dy, None, s, g, mean, rstd, p, seed, want_dbias=False)
        return (ds if has_x else None), da, dg, db, None, None, None


class BiasGeluDropoutFn(torch.autograd.Function):
    """g = dropout(gelu(h + bias)), exact-erf gelu; bias f32."""

    @staticmethod
    def forward(ctx, h, bias, p, seed):
        b = _f32(bias)
        h = h.contiguous()
        ctx.save_for_backward(h, b)
        ctx.cfg = (float(p), int(seed))
        return gelu_fwd(h, b, p, seed)

    @staticmethod
    def backward(ctx, dg):
        h, b = ctx.saved_tensors
        p, seed = ctx.cfg
        dh, dbias = gelu_bwd(dg, h, b, p, seed, want_dbias=True)
        return dh, dbias, None, None


def recurrent_cla_step(qkv, S, Z, H, eps=CLA_EPS):
    """qkv (N, 3*H*64) fused projections of ONE token per sequence; S (N, H, 64, 64), Z (N, H, 64) f32 states,
    updated in place.  -> (N, H*64)."""
    N, W = qkv.shape
    D = W // 3
    qkv = qkv.contiguous()
    out = torch.empty((N, D), dtype=qkv.dtype, device=qkv.device)
    esz = qkv.element_size()
    base = qkv.data_ptr()
    import ctypes
    _call("cwlt_recurrent_cla_step", ctypes.c_void_p(base), ctypes.c_void_p(base + D * esz),
          ctypes.c_void_p(base + 2 * D * esz), _lib.dev(S, "S"), _lib.dev(Z, "Z"), _lib.dev(out), N, H, D // H,
          W, W, W, D, float(eps), _lib.dtype_code(qkv.dtype), _lib.stream_ptr())
    return out


def cla_fwd_state(q, k, v, S, Z, lengths=None, eps=CLA_EPS, out=None, segments=None, cu=None):
    """The prompt form of recurrent_cla_step (csrc/prefill.hip): q, k, v (N, L, H, 64) views (row-strided ok) of a
    whole prompt per sequence; S (N, H, 64, 64), Z (N, H, 64) f32 recurrent states, read as the starting state and
    updated IN PLACE to the state after each sequence's last token; lengths: (N) int32 device tensor (or None = all
    L) -- rows t >= lengths[n] add nothing and stay unwritten in `out` (a dense (N, L, H, 64) buffer to write into,
    or None for a fresh one).  segments: runs per sequence of the few-stream form (None = the library's choice,
    cwlt_prefill_segments; 1 = one workgroup per (sequence, head)).  -> out.
    cu (SeqOffsets or n_songs + 1 offsets): songs laid end to end (_check_qkv; f32 views, so the three column blocks of a
    qkv buffer go in as they are), S and Z one state per song.  One workgroup per (song, head) from the song's own row 0,
    never segmented and without lengths: a song's out rows, S and Z are bitwise those of this call on it alone (N = 1,
    segments = 1).  `out` may then be a view with dense rows."""
    packed, n = ("", "N") if cu is None else ("_packed", "n_songs")
    cu, N, L, H, D = _check_qkv("cla_fwd_state" + packed, q, k, v, cu)
    if S.shape != (N, H, D, D) or Z.shape != (N, H, D):
        raise ValueError("state shapes %s / %s do not match (%s, H, D, D) / (%s, H, D) = %s"
                         % (tuple(S.shape), tuple(Z.shape), n, n, (N, H, D, D)))
    if S.dtype != torch.float32 or Z.dtype != torch.float32 or not S.is_contiguous() or not Z.is_contiguous():
        raise TypeError("the recurrent state is dense f32 (it is updated in place)")
    if lengths is not None:
        if cu is not None or lengths.shape != (N,) or lengths.dtype != torch.int32 or not lengths.is_contiguous():
            raise ValueError("lengths must be a dense (N,) int32 tensor (and the packed form takes none)")
    table = ("lengths", lengths) if cu is None else ("cu_seqlens", cu.dev)
    for name, t in (("k", k), ("v", v), ("S", S), ("Z", Z), table):
        if t is not None and t.device != q.device:
            raise ValueError("%s is on %s, q on %s" % (name, t.device, q.device))
    q, ldq = _as_rows(q)
    k, ldk = _as_rows(k)
    v, ldv = _as_rows(v)
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != q.dtype or out.device != q.device:
        raise ValueError("out must be a tensor of q's shape, dtype and device")
    elif cu is None and not out.is_contiguous():
        raise ValueError("out must be a dense (N, L, H, D) tensor")
    elif cu is not None and (out.stride(-1) != 1 or out.stride(-2) != D or out.stride(-3) < H * D):
        raise ValueError("out must be an (R, H, D) tensor with dense rows")
    lib = _lib.load()
    P = 1 if cu is not None else lib.cwlt_prefill_segments(N, H, L) if segments is None else int(segments)
    ws = torch.empty(int(lib.cwlt_prefill_seg_floats(N, H, P)), dtype=torch.float32, device=q.device) if P > 1 else None
    # the two entry points differ in their name, in how they say where the sequences are, and in out's row stride
    where, ldo, seg = (((_lib.opt(lengths), N, H, L, D), H * D, (P, _lib.opt(ws))) if cu is None
                       else ((_lib.dev(cu.dev), N, H, D), out.stride(-3), ()))
    _call("cwlt_causal_linear_fwd_state" + packed, _lib.dev(q, "q"), _lib.dev(k, "k"), _lib.dev(v, "v"), _lib.dev(out),
          _lib.dev(S, "S"), _lib.dev(Z, "Z"), *where, ldq, ldk, ldv, ldo, float(eps), *seg, _lib.dtype_code(q.dtype),
          _lib.stream_ptr())
    return out


def cla_fwd_state_packed(q, k, v, S, Z, cu, eps=CLA_EPS, out=None):
    """`cla_fwd_state(cu=cu)`: q, k, v, out (R, H, 64), S (n_songs, H, 64, 64), Z (n_songs, H, 64)."""
    return cla_fwd_state(q, k, v, S, Z, None, eps, out, cu=cu)


def sqrt_width(w):
    return math.sqrt(w)


# --------------------------------------------------------------------------------------------------
# generation: the decode step's GEMV building block (csrc/decode.hip); the whole step is generation.DecodeSession
# --------------------------------------------------------------------------------------------------
def decode_gemv(w, bias, x, ln=None, ln2=None, eps=1e-5, res=None, act=None, want_normed=False):
    """out[n] = epi(W . pro(x[n]) + bias): pro = LayerNorm(*ln) then LayerNorm(*ln2) when given; epi = exact GELU when
    act == "gelu", then + res[n].  x (n, K) f32, w (n_out, K) f32 -> (n, n_out) f32 [, the normalised x]."""
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise TypeError("decode_gemv computes in f32")
    n, K = x.shape
    n_out = w.shape[0]
    x, w = x.contiguous(), w.contiguous()
    out = torch.empty((n, n_out), dtype=torch.float32, device=x.device)
    xn = torch.empty_like(x) if (want_normed and ln is not None) else None
    if res is not None:
        res = res.contiguous()
    p = lambda pair, i: _lib.opt(None if pair is None else pair[i].contiguous())
    _call("cwlt_decode_gemv", _lib.dev(w, "w"), _lib.opt(bias), _lib.dev(x, "x"), p(ln, 0), p(ln, 1), p(ln2, 0),
          p(ln2, 1), float(eps), _lib.opt(res), _lib.dev(out), _lib.opt(xn), n_out, K, 1 if act == "gelu" else 0, n,
          K, n_out, n_out, K, _lib.stream_ptr())
    return (out, xn) if want_normed else out


def decode_gemm(w, bias, x, ln=None, ln2=None, eps=1e-5, res=None, act=None, want_normed=False, out=None,
                normed=None):
    """decode_gemv's product for many rows at once (csrc/decode_gemm.hip: f32 MFMA, each weight read once per 64 rows,
    bitwise batch invariant).  x (n, K) f32 with a row stride that is a multiple of 4, w (n_out, K) f32, K % 16 == 0
    -> (n, n_out) f32 [, the normalised x].  out / normed: row-strided (n, n_out) / (n, K) f32 views to write the
    result / the normalised x into (normed implies want_normed; its row stride a multiple of 4)."""
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise TypeError("decode_gemm computes in f32")
    n, K = x.shape
    n_out = w.shape[0]
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    w = w.contiguous()
    if out is None:
        out = torch.empty((n, n_out), dtype=torch.float32, device=x.device)
    elif out.shape != (n, n_out) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != x.device:
        raise ValueError("decode_gemm: out must be an f32 (%d, %d) view with unit column stride" % (n, n_out))
    if normed is not None:
        if ln is None or normed.shape != (n, K) or normed.dtype != torch.float32 or normed.stride(1) != 1 or \
                normed.stride(0) % 4 or normed.device != x.device:
            raise ValueError("decode_gemm: normed needs a LayerNorm prologue and an f32 (%d, %d) view, row stride % 4"
                             % (n, K))
        want_normed = True
    xn = normed if normed is not None else \
        (torch.empty((n, K), dtype=torch.float32, device=x.device) if (want_normed and ln is not None) else None)
    if res is not None and res.stride(1) != 1:
        res = res.contiguous()
    lib = _lib.load()
    need = lib.cwlt_decode_gemm_scratch_floats(n_out, K, n)
    if need < 0:
        raise ValueError("decode_gemm: unsupported shape n=%d, K=%d, n_out=%d" % (n, K, n_out))
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
    p = lambda pair, i: _lib.opt(None if pair is None else pair[i].contiguous())
    _call("cwlt_decode_gemm", _lib.dev(w, "w"), _lib.opt(bias), _lib.dev(x, "x"), p(ln, 0), p(ln, 1), p(ln2, 0),
          p(ln2, 1), float(eps), _lib.opt(res), _lib.dev(out), _lib.opt(xn), n_out, K, 1 if act == "gelu" else 0, n,
          x.stride(0), 0 if res is None else res.stride(0), out.stride(0), K if xn is None else xn.stride(0),
          _lib.dev(scratch), _lib.stream_ptr())
    return (out, xn) if want_normed else out


def _sampler_head(fn, logits, n_class, ids, temperature, top_p, what="tokens"):
    """The checks every sampler / scorer wrapper `fn` starts with -> (logits with a unit column stride, rows, A, the
    temperature and top_p float arrays (None: off; a None top_p entry is 1)).  ids: the (rows, A) int64 `what` (None: an
    entry without one)."""
    if logits.dtype != torch.float32 or (ids is not None and ids.dtype != torch.int64):
        raise TypeError("%s takes f32 logits and int64 %s" % (fn, what))
    rows, A = logits.shape[0], len(n_class)
    if ids is not None and (ids.numel() != rows * A or not ids.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous (rows, n_attr) int64 buffer" % (fn, what))
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    temp = None if temperature is None else (ctypes.c_float * A)(*[float(t) for t in temperature])
    topp = None if top_p is None else (ctypes.c_float * A)(*[1.0 if p is None else float(p) for p in top_p])
    return logits, rows, A, temp, topp


def _row_keys(fn, rows, key, step, counter=None, counted=True):
    """The row keying rule of the samplers: key and step together, (rows,) int64 each, or -- where `fn` takes a counter
    (counted) -- the slot and that counter."""
    if (key is None) != (step is None) or (key is None and (counter is None or not counted)):
        raise ValueError("%s is keyed by key and step%s" % (fn, ", or by the slot and a counter" if counted else ""))
    for t in ([] if key is None else [key, step]):
        if t.dtype != torch.int64 or t.numel() != rows or not t.is_contiguous():
            raise ValueError("%s: key and step must be contiguous (rows,) int64 tensors" % fn)


def _logp_ring(logp, rows, A, out_counter):
    """Checks of the optional (R, rows, A, 2) f32 log-prob ring -> R (1 without a ring)."""
    if logp is None:
        return 1
    if logp.dtype != torch.float32 or logp.dim() != 4 or tuple(logp.shape[1:]) != (rows, A, 2) or \
            not logp.is_contiguous():
        raise ValueError("logp must be a contiguous (R, %d, %d, 2) f32 ring" % (rows, A))
    if out_counter is None and logp.shape[0] != 1:
        raise ValueError("a logp ring of %d rows needs out_counter" % logp.shape[0])
    return logp.shape[0]


def _mask_table(n_class, rows, bar, sched, masks, key=None):
    """Checks of the optional constraint table -> (bar, sched, n_sched, masks, rows, words) ctypes arguments (all NULL /
    0 when unmasked).  key: the scorers' song index per row, checked like bar."""
    if bar is None and sched is None and masks is None:
        return None, None, 0, None, 0, 0
    if bar is None or sched is None or masks is None:
        raise ValueError("the constraint table needs bar, sched and masks together")
    for t in [bar] + ([] if key is None else [key]):
        if t.dtype != torch.int64 or t.numel() != rows or not t.is_contiguous():
            raise ValueError("bar and key must be contiguous (rows,) int64 tensors")
    if sched.dtype != torch.int64 or sched.dim() != 2 or sched.shape[1] != 2 or not sched.is_contiguous():
        raise ValueError("sched must be a contiguous (n_songs, 2) int64 tensor")
    if masks.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or masks.dim() != 2 or \
            not masks.is_contiguous():
        raise ValueError("masks must be a contiguous (rows, words) 32-bit tensor")
    if masks.shape[1] * 32 < sum(n_class):
        raise ValueError("masks: %d words per row hold fewer than the %d classes" % (masks.shape[1], sum(n_class)))
    return (_lib.dev(bar, "bar"), _lib.dev(sched, "sched"), sched.shape[0], _lib.dev(masks, "masks"), masks.shape[0],
            masks.shape[1])


def _grammar_table(n_class, rows, beat, order, gram, bar_attr):
    """Checks of the row grammar's device tables -> (beat, order, n_order, gram, words, bar_attr) ctypes arguments."""
    if beat.dtype != torch.int64 or beat.numel() != rows or not beat.is_contiguous():
        raise ValueError("beat must be a contiguous (rows,) int64 tensor")
    if not 0 <= int(bar_attr) < len(n_class):
        raise ValueError("bar_attr %d outside the %d attributes" % (bar_attr, len(n_class)))
    if order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous() or \
            order.numel() < n_class[int(bar_attr)]:
        raise ValueError("order must be a contiguous int32 tensor of >= %d entries" % n_class[int(bar_attr)])
    if gram.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or gram.dim() != 2 or \
            gram.shape[0] != 3 or not gram.is_contiguous():
        raise ValueError("gram must be a contiguous (3, words) 32-bit tensor")
    if gram.shape[1] * 32 < sum(n_class):
        raise ValueError("gram: %d words per row hold fewer than the %d classes" % (gram.shape[1], sum(n_class)))
    return (_lib.dev(beat, "beat"), _lib.dev(order, "order"), order.numel(), _lib.dev(gram, "gram"), gram.shape[1],
            int(bar_attr))


def sample_categorical(logits, n_class, tokens, seed, counter=None, song=None, temperature=None, top_p=None,
                       slot_keys=False):
    """tokens[row, a] ~ Categorical(softmax(logits[row, segment a] / temperature[a])) on the device
    (csrc/sample.hip; ppo_policy/inference.py:115-141).  logits (rows, >= sum n_class) f32; tokens (rows, A) int64
    written in place; counter: device int64 scalar tensor that keys the draw (and indexes `song` (T, rows, A));
    top_p[a] < 1 (or None = off) samples attribute a from its nucleus (dqn_policy/model.py:33-47).
    slot_keys=True: the draw of row n does not depend on `rows` (cwlt_sample_categorical_slots; same draws at rows == 1)."""
    logits, rows, A, temp, topp = _sampler_head("sample_categorical", logits, n_class, tokens, temperature, top_p)
    _call("cwlt_sample_categorical_slots" if slot_keys else "cwlt_sample_categorical", _lib.dev(logits, "logits"),
          _lib.int_array(n_class), temp, topp, A, rows, logits.stride(0), int(seed) & 0xFFFFFFFFFFFFFFFF,
          _lib.opt(counter), _lib.dev(tokens, "tokens"), _lib.opt(song), 0 if song is None else song.shape[0],
          _lib.stream_ptr())
    return tokens


# --------------------------------------------------------------------------------------------------
# continuous batching (csrc/stream.hip, csrc/sample.hip): the per-token launches of generation.generate_stream
# --------------------------------------------------------------------------------------------------
def sample_categorical_keyed(logits, n_class, tokens, seed, key, step, temperature=None, top_p=None):
    """sample_categorical with per-row keys: row n draws what slot_keys=True draws for row key[n] at counter step[n]
    (cwlt_sample_categorical_keyed).  key, step: (rows,) int64 device tensors (song index < 2^20, position < 2^40)."""
    fn = "sample_categorical_keyed"
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, tokens, temperature, top_p)
    _row_keys(fn, rows, key, step, counted=False)
    _call("cwlt_sample_categorical_keyed", _lib.dev(logits, "logits"), _lib.int_array(n_class), temp, topp, A, rows,
          logits.stride(0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.dev(key, "key"), _lib.dev(step, "step"),
          _lib.dev(tokens, "tokens"), _lib.stream_ptr())
    return tokens


def sample_categorical_masked(logits, n_class, tokens, seed, bar, sched, masks, counter=None, key=None, step=None,
                              temperature=None, top_p=None):
    """The constrained draw (cwlt_sample_categorical_masked): sample_categorical(slot_keys=True) at `counter` (song k =
    row n) or sample_categorical_keyed with per-row key / step (song k = key[n]), with every class whose bit is clear
    in the song's mask row treated as a -inf logit.  bar (rows,) int64: the song's bar count before this row; sched
    (n_sched, 2) int64: per song index {first mask row, rows}, row used first + min(bar - 1, rows - 1); masks
    (mask_rows, mask_words) int32 / uint32 bits, class c of attribute a at bit sum(n_class[:a]) + c.  Songs k < 0 or
    >= n_sched and 0-row schedules draw unmasked.  All device tensors."""
    fn = "sample_categorical_masked"
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, tokens, temperature, top_p)
    _row_keys(fn, rows, key, step, counter)
    if bar is None:
        raise ValueError("%s needs the constraint table: bar, sched and masks" % fn)
    table = _mask_table(n_class, rows, bar, sched, masks)
    _call("cwlt_sample_categorical_masked", _lib.dev(logits, "logits"), _lib.int_array(n_class), temp, topp, A, rows,
          logits.stride(0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.opt(counter), _lib.opt(key), _lib.opt(step), *table,
          _lib.dev(tokens, "tokens"), _lib.stream_ptr())
    return tokens


def sample_categorical_logp(logits, n_class, tokens, seed, logp, counter=None, key=None, step=None, bar=None,
                            sched=None, masks=None, out_counter=None, temperature=None, top_p=None):
    """The draw of sample_categorical(slot_keys=True) at `counter`, or of sample_categorical_keyed with key / step,
    masked as sample_categorical_masked when bar / sched / masks are given -- the same tokens -- that also writes the
    (model, sampler) log-probs of each drawn class (cwlt_sample_categorical_logp).  logp: (R, rows, A, 2)
    f32 device ring; the pair of row n, attribute a goes to logp[*out_counter % R, n, a] (out_counter: device int64,
    e.g. the counter the loop advances after the draw; None needs R == 1)."""
    fn = "sample_categorical_logp"
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, tokens, temperature, top_p)
    _row_keys(fn, rows, key, step, counter)
    R = _logp_ring(logp, rows, A, out_counter)
    table = _mask_table(n_class, rows, bar, sched, masks)
    _call("cwlt_sample_categorical_logp", _lib.dev(logits, "logits"), _lib.int_array(n_class), temp, topp, A, rows,
          logits.stride(0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.opt(counter), _lib.opt(key), _lib.opt(step), *table,
          _lib.dev(tokens, "tokens"), _lib.dev(logp, "logp"), _lib.opt(out_counter), R, _lib.stream_ptr())
    return tokens


def sample_categorical_grammar(logits, n_class, tokens, seed, beat, order, gram, bar_attr=2, counter=None, key=None,
                               step=None, bar=None, sched=None, masks=None, logp=None, out_counter=None,
                               temperature=None, top_p=None):
    """The draw under the row grammar (cwlt_sample_categorical_grammar): keyed as
    sample_categorical_logp (slot and `counter`, or key / step), masked by bar / sched / masks when given, the bar-beat
    class (attribute bar_attr) drawn first under the position rule -- beat (rows,) int64, order (>= n_class[bar_attr],)
    int32 -- and every other attribute under the row of gram (3, words) its kind selects.  logp (optional): the (R, rows,
    A, 2) f32 ring of sample_categorical_logp, row *out_counter % R."""
    fn = "sample_categorical_grammar"
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, tokens, temperature, top_p)
    _row_keys(fn, rows, key, step, counter)
    R = _logp_ring(logp, rows, A, out_counter)
    table = _mask_table(n_class, rows, bar, sched, masks)
    gtable = _grammar_table(n_class, rows, beat, order, gram, bar_attr)
    _call("cwlt_sample_categorical_grammar", _lib.dev(logits, "logits"), _lib.int_array(n_class), temp, topp, A, rows,
          logits.stride(0), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.opt(counter), _lib.opt(key), _lib.opt(step), *table,
          *gtable, _lib.dev(tokens, "tokens"), _lib.opt(logp), _lib.opt(out_counter), R, _lib.stream_ptr())
    return tokens


def _rows(t, a, z):
    """Rows a .. z of a per-row tensor; None stays None."""
    return None if t is None else t[a:z]


def _table_slices(n_class, rows, key, bar, sched, masks, grammar, no_grammar=()):
    """The body the scorers and policy_stats share: the checks of the constraint table and of grammar = (beat, order,
    gram, bar_attr) (None: none) on all rows, then -- a generator -- per launch of at most 2^20 rows (a, z, key, table,
    gtable): the rows a .. z, their slice of key (None without keys) and the two tables' ctypes arguments for them;
    gtable is no_grammar without a grammar."""
    if key is not None and bar is None:
        raise ValueError("key selects a song's constraint row: it needs bar, sched and masks")
    _mask_table(n_class, rows, bar, sched, masks, key)
    if grammar is not None:
        beat, order, gram, bar_attr = grammar
        _grammar_table(n_class, rows, beat, order, gram, bar_attr)

    def slices():
        for a in range(0, rows, 1 << 20):
            z = min(rows, a + (1 << 20))
            k = _rows(key, a, z)
            yield (a, z, k, _mask_table(n_class, z - a, _rows(bar, a, z), sched, masks, k), no_grammar if grammar is None
                   else _grammar_table(n_class, z - a, beat[a:z], order, gram, bar_attr))
    return slices()


def _score(fn, logits, n_class, targets, temperature, top_p, key, bar, sched, masks, out, grammar=None):
    """The scorers' body: the checks on all rows, then launches of at most 2^20 rows of cwlt_<fn>.  grammar: (beat, order,
    gram, bar_attr) for the grammar entry, whose arguments follow the constraint table's."""
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, targets, temperature, top_p, "targets")
    slices = _table_slices(n_class, rows, key, bar, sched, masks, grammar)
    if out is None:
        out = torch.empty((rows, A, 2), dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, A, 2) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (%d, %d, 2) f32 tensor" % (rows, A))
    tv = targets.view(rows, A)
    for a, z, k, table, gtable in slices:
        _call("cwlt_" + fn, _lib.dev(logits[a:z], "logits"), _lib.int_array(n_class), temp, topp, A, z - a,
              logits.stride(0), _lib.dev(tv[a:z], "targets"), _lib.opt(k), *table, *gtable,
              _lib.dev(out[a:z], "logp"), _lib.stream_ptr())
    return out


def score_categorical(logits, n_class, targets, temperature=None, top_p=None, key=None, bar=None, sched=None,
                      masks=None, out=None):
    """(model, sampler) log-probs of given classes (cwlt_score_categorical): logits (rows, >= sum n_class)
    f32, targets (rows, A) int64 (negative: padding, left unwritten) -> (rows, A, 2) f32.  Masked when bar / sched /
    masks are given, song key[n] (None: n).  Bitwise the pairs sample_categorical_logp writes for the same logits,
    settings and classes.  Rows go through in launches of at most 2^20."""
    return _score("score_categorical", logits, n_class, targets, temperature, top_p, key, bar, sched, masks, out)


def score_categorical_grammar(logits, n_class, targets, beat, order, gram, bar_attr=2, temperature=None, top_p=None,
                              key=None, bar=None, sched=None, masks=None, out=None):
    """score_categorical under the row grammar (cwlt_score_categorical_grammar): the kind of row n is that of its
    target's bar-beat class, beat (rows,) int64 the position before each row -> (rows, A, 2) f32."""
    return _score("score_categorical_grammar", logits, n_class, targets, temperature, top_p, key, bar, sched, masks,
                  out, (beat, order, gram, bar_attr))


def policy_stats(logits, n_class, ref_logits=None, temperature=None, top_p=None, key=None, bar=None, sched=None,
                 masks=None, bar_class=None, grammar=None, out=None):
    """Entropy of the model's and of the sampler's distribution per row and attribute, and with ref_logits (a second
    model's logits for the same rows, its own row stride) their KL against the reference's (cwlt_policy_stats, DESIGN
    §4.6i): logits (rows, >= sum n_class) f32 -> (rows, A, 2) f32 {H(p), H(q)} or (rows, A, 4) {H(p), H(q), KL(p || p'),
    KL(q || q')} in nats.  p = softmax(logits); q what score_categorical(_grammar) scores the row under: temperature,
    top_p, the constraint table (key / bar / sched / masks) and grammar = (beat, order, gram, bar_attr).  bar_class
    (rows,) int64: the row's own bar-beat class -- negative: padding, left unwritten; it fixes the row's kind under a
    grammar, which needs it.  KL(q || q') is +inf where q's kept set is not inside q''s; a row with no allowed class has
    NaN in the q columns.  Rows go through in launches of at most 2^20."""
    fn = "policy_stats"
    rows, A = logits.shape[0], len(n_class)
    logits, rows, A, temp, topp = _sampler_head(fn, logits, n_class, None, temperature, top_p)
    if logits.dim() != 2 or logits.shape[1] < sum(n_class):
        raise ValueError("%s: logits must be (rows, >= %d)" % (fn, sum(n_class)))
    if bar_class is None:
        if grammar is not None:
            raise ValueError("%s: a grammar needs bar_class, the row's own bar-beat class" % fn)
    elif bar_class.dtype != torch.int64 or bar_class.numel() != rows or not bar_class.is_contiguous():
        raise ValueError("%s: bar_class must be a contiguous (rows,) int64 tensor" % fn)
    C = 2
    if ref_logits is not None:
        if ref_logits.dtype != torch.float32 or ref_logits.dim() != 2 or ref_logits.shape[0] != rows or \
                ref_logits.shape[1] < sum(n_class) or ref_logits.device != logits.device:
            raise ValueError("%s: ref_logits must be (%d, >= %d) f32 on the logits' device" % (fn, rows, sum(n_class)))
        if ref_logits.stride(-1) != 1:
            ref_logits = ref_logits.contiguous()
        C = 4
    slices = _table_slices(n_class, rows, key, bar, sched, masks, grammar, (None, None, 0, None, 0, 0))
    if out is None:
        out = torch.empty((rows, A, C), dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows, A, C) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (%d, %d, %d) f32 tensor" % (rows, A, C))
    for a, z, k, table, gtable in slices:
        _call("cwlt_policy_stats", _lib.dev(logits[a:z], "logits"), _lib.int_array(n_class), temp, topp, A, z - a,
              logits.stride(0), _lib.opt(_rows(ref_logits, a, z)), 0 if ref_logits is None else ref_logits.stride(0),
              _lib.opt(_rows(bar_class, a, z)), _lib.opt(k), *table, *gtable, _lib.dev(out[a:z], "out"),
              _lib.stream_ptr())
    return out


def blend_logits(logits, ref_logits, n_class, alpha, key=None, out=None):
    """out = alpha logits + (1 - alpha) ref_logits, attribute by attribute (cwlt_blend_logits): the logits
    of pi^alpha pi_ref^(1 - alpha).  logits, ref_logits (rows, >= sum n_class) f32 with unit column strides and row
    strides of their own; alpha (n_alpha, A) f32 on the device: row 0 when n_alpha == 1, else row key[n] ((rows,) int64;
    None: n), a row whose key is outside [0, n_alpha) copied from logits.  out: None (a new (rows, sum n_class) tensor),
    `logits` itself (in place), or a tensor that overlaps neither input; columns past sum n_class are left alone.
    alpha = 1 returns logits and alpha = 0 ref_logits exactly.  Rows go through in launches of at most 2^20."""
    fn, W, A = "blend_logits", sum(n_class), len(n_class)
    for t, name in ((logits, "logits"), (ref_logits, "ref_logits")) + (() if out is None else ((out, "out"),)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < W or t.stride(1) != 1 or \
                t.shape[0] != logits.shape[0] or t.device != logits.device:
            raise ValueError("%s: %s must be (%d, >= %d) f32 with a unit column stride on the logits' device"
                             % (fn, name, logits.shape[0], W))
    rows = logits.shape[0]
    if alpha.dtype != torch.float32 or alpha.dim() != 2 or alpha.shape[1] != A or alpha.shape[0] < 1 or \
            not alpha.is_contiguous():
        raise ValueError("%s: alpha must be a contiguous (n_alpha, %d) f32 tensor" % (fn, A))
    if key is not None and (key.dtype != torch.int64 or key.numel() != rows or not key.is_contiguous()):
        raise ValueError("%s: key must be a contiguous (rows,) int64 tensor" % fn)
    if key is None and alpha.shape[0] not in (1, rows):
        raise ValueError("%s: without a key alpha has one row or one per row (%d), got %d" % (fn, rows, alpha.shape[0]))
    if out is None:
        out = torch.empty((rows, W), dtype=torch.float32, device=logits.device)
    for a in range(0, rows, 1 << 20):
        z = min(rows, a + (1 << 20))
        # without a key the alpha row of row n is n: a later launch starts at its own rows of the table
        al = alpha if key is not None or alpha.shape[0] == 1 else alpha[a:z]
        _call("cwlt_blend_logits", _lib.dev(logits[a:z], "logits"), logits.stride(0),
              _lib.dev(ref_logits[a:z], "ref_logits"), ref_logits.stride(0), _lib.int_array(n_class), A,
              _lib.dev(al, "alpha"), al.shape[0], _lib.opt(_rows(key, a, z)), _lib.dev(out[a:z], "out"), out.stride(0),
              z - a, _lib.stream_ptr())
    return out


def _prefer_pen(fn, pen, A):
    """Checks of the penalty table (n_songs, 2 A + 1) f32 -> n_songs."""
    if pen.dtype != torch.float32 or pen.dim() != 2 or pen.shape[1] != 2 * A + 1 or pen.shape[0] < 1 or \
            not pen.is_contiguous():
        raise ValueError("%s: pen must be a contiguous (n_songs, %d) f32 tensor" % (fn, 2 * A + 1))
    return pen.shape[0]


def _prefer_seen(fn, seen, rows, W, name="seen"):
    if seen.dtype != torch.float32 or seen.dim() != 2 or seen.shape[0] != rows or seen.shape[1] < W or \
            seen.stride(1) != 1:
        raise ValueError("%s: %s must be (%d, >= %d) f32 with a unit column stride" % (fn, name, rows, W))


def prefer_logits(logits, n_class, sched=None, bias=None, pen=None, seen=None, key=None, bar=None, out=None):
    """The preferred logits (cwlt_prefer_logits): out[n, c] = ((logits[n, c] + b) - f s) - (s > 0 ? p :
    0).  logits (rows, >= sum n_class) f32, unit column stride.  sched (n_songs, 2) int64 {first bias row, rows} with
    bias (R, >= sum n_class) f32, R >= 1, together or not at all; pen (n_songs, 2 A + 1) f32 {frequency, presence,
    decay} with seen (rows, >= sum n_class) f32 (seen None: no penalty).  key (rows,) int64: the song of each row (None:
    row n is song n), a row whose song is outside [0, n_songs) is copied; bar (rows,) int64: the bar count that picks
    the bias row as the masked sampler picks its mask row (None: the first row).  out: None (a new tensor), `logits`
    (in place) or a tensor that overlaps no input.  Rows go through in launches of at most 2^20."""
    fn, W, A = "prefer_logits", sum(n_class), len(n_class)
    for t, name in ((logits, "logits"),) + (() if out is None else ((out, "out"),)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < W or t.stride(1) != 1 or \
                t.shape[0] != logits.shape[0] or t.device != logits.device:
            raise ValueError("%s: %s must be (%d, >= %d) f32 with a unit column stride on the logits' device"
                             % (fn, name, logits.shape[0], W))
    rows = logits.shape[0]
    if (sched is None) != (bias is None):
        raise ValueError("%s: sched and bias go together" % fn)
    if sched is None and pen is None:
        raise ValueError("%s needs a bias table (sched, bias), a penalty table (pen), or both" % fn)
    n_songs = None
    if sched is not None:
        if sched.dtype != torch.int64 or sched.dim() != 2 or sched.shape[1] != 2 or sched.shape[0] < 1 or \
                not sched.is_contiguous():
            raise ValueError("%s: sched must be a contiguous (n_songs, 2) int64 tensor" % fn)
        if bias.dtype != torch.float32 or bias.dim() != 2 or bias.shape[0] < 1 or bias.shape[1] < W or \
                bias.stride(1) != 1:
            raise ValueError("%s: bias must be (R >= 1, >= %d) f32 with a unit column stride" % (fn, W))
        n_songs = sched.shape[0]
    if seen is not None and pen is None:
        raise ValueError("%s: seen needs the penalty table pen" % fn)
    if pen is not None:
        n_pen = _prefer_pen(fn, pen, A)
        if n_songs is not None and n_pen != n_songs:
            raise ValueError("%s: pen has %d rows, sched %d" % (fn, n_pen, n_songs))
        n_songs = n_pen
    if seen is not None:
        _prefer_seen(fn, seen, rows, W)
    for t, name in ((key, "key"), (bar, "bar")):
        if t is not None and (t.dtype != torch.int64 or t.numel() != rows or not t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous (rows,) int64 tensor" % (fn, name))
    if key is None and rows > 1 << 20:
        raise ValueError("%s: without a key row n is song n of one launch: more than 2^20 rows need a key" % fn)
    if out is None:
        out = torch.empty((rows, W), dtype=torch.float32, device=logits.device)
    for a in range(0, rows, 1 << 20):
        z = min(rows, a + (1 << 20))
        _call("cwlt_prefer_logits", _lib.dev(logits[a:z], "logits"), logits.stride(0), _lib.int_array(n_class), A,
              _lib.opt(_rows(key, a, z)), _lib.opt(_rows(bar, a, z)), _lib.opt(sched), n_songs, _lib.opt(bias),
              0 if bias is None else bias.shape[0], 0 if bias is None else bias.stride(0), _lib.opt(pen),
              _lib.opt(_rows(seen, a, z)), 0 if seen is None else seen.stride(0), _lib.dev(out[a:z], "out"),
              out.stride(0), z - a, _lib.stream_ptr())
    return out


def prefer_track(tokens, n_class, pen, seen, fresh=None, song=None, seen0=None):
    """The repetition state after a draw (cwlt_prefer_track): seen[n] (rows, >= sum n_class) f32 becomes seen[n] * decay
    + hit, hit 1 at the class tokens (rows, A) int64 carries in each attribute, decay from row song[n] (None: n) of pen
    (n_songs, 2 A + 1) f32.  With fresh / song (rows,) int64 and seen0 (n_songs, sum n_class) f32, a row flagged fresh
    with song >= 0 takes seen0[song] instead; a row whose song is outside [0, n_songs) is left alone."""
    fn, W, A = "prefer_track", sum(n_class), len(n_class)
    if tokens.dtype != torch.int64 or not tokens.is_contiguous() or tokens.shape[-1] != A or seen.dim() != 2 or \
            tokens.numel() != seen.shape[0] * A:
        raise TypeError("%s takes contiguous int64 tokens (rows, %d) and seen (rows, >= %d)" % (fn, A, W))
    rows = seen.shape[0]
    if rows < 1 or rows > 1 << 20:
        raise ValueError("%s: 1 .. 2^20 rows, got %d" % (fn, rows))
    _prefer_seen(fn, seen, rows, W)
    n_songs = _prefer_pen(fn, pen, A)
    opt = [fresh, song, seen0]
    if any(t is not None for t in opt):
        if any(t is None or not t.is_contiguous() for t in opt) or fresh.dtype != torch.int64 or \
                song.dtype != torch.int64 or fresh.numel() != rows or song.numel() != rows or \
                seen0.dtype != torch.float32 or tuple(seen0.shape) != (n_songs, W):
            raise ValueError("%s: fresh and song (rows,) int64 and seen0 (n_songs, %d) f32 go together" % (fn, W))
    _call("cwlt_prefer_track", _lib.dev(tokens, "tokens"), rows, _lib.int_array(n_class), A, _lib.dev(pen, "pen"),
          n_songs, _lib.opt(fresh), _lib.opt(song), _lib.opt(seen0), _lib.dev(seen, "seen"), seen.stride(0),
          _lib.stream_ptr())
    return seen


def prefer_scan(tokens, n_songs_block, n_class, pen, key=None, out=None, cu=None):
    """The repetition state along given songs (cwlt_prefer_scan): tokens (nb * Lb, A) int64, song i in rows [i Lb,
    (i + 1) Lb) -> seen_rows (nb * Lb, sum n_class) f32, row t of a song the state after its rows 0 .. t from zero, by
    prefer_track's step with the decay of song key[i Lb] (key (nb * Lb,) int64, the per-row key of prefer_logits; None:
    song i) in pen (n_songs, 2 A + 1) f32.  Songs go through in launches of at most 2^20 rows.
    cu (SeqOffsets or n + 1 offsets; n_songs_block is then unused): songs laid end to end (cwlt_prefer_scan_packed),
    song i in rows [cu[i], cu[i + 1]) with the decay of song key[cu[i]], every song's rows bitwise the above."""
    fn, W, A = "prefer_scan" if cu is None else "prefer_scan_packed", sum(n_class), len(n_class)
    if tokens.dtype != torch.int64 or not tokens.is_contiguous() or tokens.dim() != 2 or tokens.shape[1] != A:
        raise TypeError("%s takes contiguous int64 tokens (rows, %d)" % (fn, A))
    total = tokens.shape[0]
    if cu is None:
        nb = int(n_songs_block)
        if nb < 1 or total < nb or total % nb:
            raise ValueError("%s: %d token rows are no whole number of rows for each of %d songs" % (fn, total, nb))
        Lb = total // nb
        if Lb > 1 << 20:
            raise ValueError("%s: a song of %d rows is past the 2^20 rows of one launch" % (fn, Lb))
    else:
        _lib.dev(tokens, "tokens")
        cu = _seq_offsets(cu, tokens.device).check_rows(total)
        nb = cu.n_songs
        if nb > 1 << 20:
            raise ValueError("%s: %d songs are past the 2^20 songs of one launch" % (fn, nb))
    n_songs = _prefer_pen(fn, pen, A)
    if key is not None and (key.dtype != torch.int64 or key.numel() != total or not key.is_contiguous()):
        raise ValueError("%s: key must be a contiguous (rows,) int64 tensor" % fn)
    if key is None and nb > n_songs:
        raise ValueError("%s: without a key song i reads row i of pen: %d songs, %d rows" % (fn, nb, n_songs))
    if out is None:
        out = torch.empty((total, W), dtype=torch.float32, device=tokens.device)
    else:
        _prefer_seen(fn, out, total, W, "out")
    if cu is not None:
        _call("cwlt_prefer_scan_packed", _lib.dev(tokens, "tokens"), _lib.dev(cu.dev), nb, _lib.int_array(n_class), A,
              _lib.dev(pen, "pen"), n_songs, _lib.opt(key), _lib.dev(out, "seen_rows"), out.stride(0), _lib.stream_ptr())
        return out
    per = max(1, (1 << 20) // Lb)
    for a in range(0, nb, per):
        z = min(nb, a + per)
        pn = pen if key is not None else pen[a:]
        _call("cwlt_prefer_scan", _lib.dev(tokens[a * Lb:z * Lb], "tokens"), z - a, Lb, _lib.int_array(n_class), A,
              _lib.dev(pn, "pen"), pn.shape[0], _lib.opt(_rows(key, a * Lb, z * Lb)),
              _lib.dev(out[a * Lb:z * Lb], "seen_rows"), out.stride(0), _lib.stream_ptr())
    return out


def prefer_scan_packed(tokens, cu, n_class, pen, key=None, out=None):
    """`prefer_scan(cu=cu)`: tokens (R, A) int64 -> seen_rows (R, sum n_class) f32."""
    return prefer_scan(tokens, None, n_class, pen, key, out, cu=cu)


def grammar_track(tokens, bar_attr, order, beat, fresh=None, song=None, beat0=None):
    """The row grammar's position after a draw (cwlt_grammar_track): beat[n] (rows,) int64 moves by the bar-beat class
    of tokens (rows, A) int64 through order (int32: -1 Bar, k >= 0 Beat_k, else unchanged); with fresh / song (rows,)
    int64 and beat0 (n_songs,) int64, a row flagged fresh with song >= 0 starts from beat0[song] instead."""
    rows, A = beat.numel(), tokens.shape[-1]
    if tokens.dtype != torch.int64 or beat.dtype != torch.int64 or not tokens.is_contiguous() or \
            not beat.is_contiguous() or tokens.numel() != rows * A:
        raise TypeError("grammar_track takes contiguous int64 tokens (rows, A) and beat (rows,)")
    if order.dtype != torch.int32 or not order.is_contiguous():
        raise TypeError("grammar_track takes a contiguous int32 order")
    opt = [fresh, song, beat0]
    if any(t is not None for t in opt):
        if any(t is None or t.dtype != torch.int64 or not t.is_contiguous() for t in opt) or \
                fresh.numel() != rows or song.numel() != rows:
            raise ValueError("grammar_track: fresh and song (rows,) and beat0 (n_songs,) int64 go together")
    _call("cwlt_grammar_track", _lib.dev(tokens, "tokens"), rows, A, int(bar_attr), _lib.dev(order, "order"),
          order.numel(), _lib.opt(fresh), _lib.opt(song), _lib.opt(beat0), 0 if beat0 is None else beat0.numel(),
          _lib.dev(beat, "beat"), _lib.stream_ptr())
    return beat


def count_bars(tokens, bar_attr, bar_mask, bar):
    """bar[n] += 1 where row n of tokens (rows, A) int64 has a Bar class in attribute bar_attr (bar_mask
    (n_class[bar_attr],) int32) -- cwlt_count_bars, the batch loop's bar count in constrained mode."""
    rows, A = bar.numel(), tokens.shape[-1]
    if tokens.dtype != torch.int64 or bar.dtype != torch.int64 or not tokens.is_contiguous() or \
            not bar.is_contiguous():
        raise TypeError("count_bars takes contiguous int64 tokens and bar")
    if bar_mask.dtype != torch.int32 or tokens.numel() != rows * A:
        raise ValueError("count_bars: tokens must be (rows, A) for %d bar counts, bar_mask int32" % rows)
    _call("cwlt_count_bars", _lib.dev(tokens, "tokens"), rows, A, int(bar_attr), _lib.dev(bar_mask, "bar_mask"),
          bar_mask.numel(), _lib.dev(bar, "bar"), _lib.stream_ptr())
    return bar


def particle_weigh(logp, out_counter, bar, bar_cond, cap, lw, length, done):
    """One token of the particles' weights (cwlt_particle_weigh): for every row n with done[n] == 0,
    lw[n] += sum_a (logp[o, n, a, 0] - logp[o, n, a, 1]) with o = *out_counter % R (logp the (R, rows, A, 2) f32 ring of
    sample_categorical_logp, out_counter its device int64 counter; None needs R == 1), length[n] += 1, and done[n] = 1
    when bar[n] >= bar_cond or length[n] >= cap[n].  lw (rows,) f32; bar, cap, length, done (rows,) int64."""
    rows = lw.numel()
    if logp.dtype != torch.float32 or lw.dtype != torch.float32 or not logp.is_contiguous() or not lw.is_contiguous():
        raise TypeError("particle_weigh takes a contiguous f32 log-prob ring and f32 weights")
    if logp.dim() != 4 or logp.shape[1] != rows or logp.shape[3] != 2:
        raise ValueError("particle_weigh: logp must be (R, rows = %d, A, 2), got %s" % (rows, tuple(logp.shape)))
    for t in (bar, cap, length, done):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != rows:
            raise TypeError("particle_weigh takes contiguous int64 bar, cap, length and done of %d rows" % rows)
    if out_counter is None and logp.shape[0] != 1:
        raise ValueError("particle_weigh: a ring of %d rows needs its counter" % logp.shape[0])
    if out_counter is not None and out_counter.dtype != torch.int64:
        raise TypeError("particle_weigh: out_counter must be a device int64")
    _call("cwlt_particle_weigh", _lib.dev(logp, "logp"), _lib.opt(out_counter), logp.shape[0], rows, logp.shape[2],
          _lib.dev(bar, "bar"), int(bar_cond), _lib.dev(cap, "cap"), _lib.dev(lw, "lw"), _lib.dev(length, "length"),
          _lib.dev(done, "done"), _lib.stream_ptr())
    return lw


def _resample_groups(fn, lw, done, particles, anc, u, ess, resampled, log_z, song=None):
    """(groups, K) of a resampling event, its per-row and per-group tensors checked (song: the keyed form's)."""
    rows, K = lw.numel(), int(particles)
    if K < 1 or rows % K:
        raise ValueError("%s: %d rows are no whole groups of %d particles" % (fn, rows, K))
    groups = rows // K
    for t, dt, n in ((lw, torch.float32, rows), (done, torch.int64, rows), (anc, torch.int64, rows),
                     (u, torch.float32, groups), (ess, torch.float32, groups), (resampled, torch.int32, groups),
                     (log_z, torch.float32, groups)) + (() if song is None else ((song, torch.int64, groups),)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise TypeError("%s takes contiguous lw f32 / done, anc int64 (rows,) and u, ess, log_z f32 / resampled "
                            "int32%s (groups,)" % (fn, "" if song is None else " / song int64"))
    return groups, K


def particle_resample(lw, done, particles, ess_frac, seed, event, anc, u, ess, resampled, log_z):
    """One resampling event (cwlt_particle_resample): lw, done (rows,) in groups of `particles` consecutive
    rows; a group below ess_frac * particles effective samples (and not all done) is resampled systematically.  Written:
    anc (rows,) int64 global ancestor rows (the identity for a kept group), u, ess (groups,) f32, resampled (groups,)
    int32; log_z (groups,) f32 gains the group's evidence increment and its lw become 0.  u is keyed by (seed, event,
    group)."""
    groups, K = _resample_groups("particle_resample", lw, done, particles, anc, u, ess, resampled, log_z)
    _call("cwlt_particle_resample", _lib.dev(lw, "lw"), _lib.dev(done, "done"), groups, K, float(ess_frac),
          int(seed) & 0xFFFFFFFFFFFFFFFF, int(event), _lib.dev(anc, "anc"), _lib.dev(u, "u"), _lib.dev(ess, "ess"),
          _lib.dev(resampled, "resampled"), _lib.dev(log_z, "log_z"), _lib.stream_ptr())
    return anc


def particle_gather(dst, src, anc, row_bytes, n_blocks=1, block_stride=0, copy_back=False):
    """dst[b][n] = src[b][anc[n]] for the rows n with anc[n] != n (cwlt_particle_gather): dst and src are
    contiguous tensors (or views: the family starts at their first element) of one layout, row n of block b at byte
    b * block_stride + n * row_bytes; anc (rows,) int64.  Rows that stay, and rows whose ancestor is out of range, are
    neither read nor written.  dst must not be src: move a state through a scratch buffer, in two calls, the second
    with copy_back=True (dst[b][n] = src[b][n] for the same rows)."""
    rows = anc.numel()
    if anc.dtype != torch.int64 or not anc.is_contiguous():
        raise TypeError("particle_gather takes a contiguous int64 ancestor vector")
    if not dst.is_contiguous() or not src.is_contiguous():
        raise TypeError("particle_gather takes contiguous buffers")
    need = (int(n_blocks) - 1) * int(block_stride) + rows * int(row_bytes)
    for t, name in ((dst, "dst"), (src, "src")):
        if t.numel() * t.element_size() < need:
            raise ValueError("particle_gather: %s holds %d bytes, the family %d (%d blocks, stride %d, %d rows x %d B)"
                             % (name, t.numel() * t.element_size(), need, n_blocks, block_stride, rows, row_bytes))
    _call("cwlt_particle_gather", _lib.dev(dst, "dst"), _lib.dev(src, "src"), _lib.dev(anc, "anc"), rows,
          int(row_bytes), int(n_blocks), int(block_stride), int(bool(copy_back)), _lib.stream_ptr())
    return dst


_INT64_ROWS = "%s: %s must be a contiguous int64 tensor of %d elements"


def _int64_rows(fn, rows, **tensors):
    """Every tensor a contiguous int64 of `rows` elements."""
    for name, t in tensors.items():
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != rows:
            raise TypeError(_INT64_ROWS % (fn, name, rows))


def particle_resample_keyed(lw, done, particles, ess_frac, seed, song, pos, every, anc, u, ess, resampled, log_z,
                            pos_stride=None):
    """particle_resample for the particle stream (cwlt_particle_resample_keyed): u is keyed by (seed, the
    song's own event index pos / every - 1, song[g]); song (groups,) int64 (< 0: no song: the group is left alone, anc
    the identity, u = ess = 0); pos int64, group g's clock at pos[g * pos_stride] (default: particles, pos per row)."""
    fn = "particle_resample_keyed"
    groups, K = _resample_groups(fn, lw, done, particles, anc, u, ess, resampled, log_z, song)
    stride = K if pos_stride is None else int(pos_stride)
    if pos.dtype != torch.int64 or not pos.is_contiguous() or stride < 1 or pos.numel() < (groups - 1) * stride + 1:
        raise TypeError("%s: pos must be a contiguous int64 tensor with group g's clock at g * %d" % (fn, stride))
    _call("cwlt_particle_resample_keyed", _lib.dev(lw, "lw"), _lib.dev(done, "done"), groups, K, float(ess_frac),
          int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.dev(song, "song"), _lib.dev(pos, "pos"), stride, int(every),
          _lib.dev(anc, "anc"), _lib.dev(u, "u"), _lib.dev(ess, "ess"), _lib.dev(resampled, "resampled"),
          _lib.dev(log_z, "log_z"), _lib.stream_ptr())
    return anc


def particle_advance(tokens, pid, done, pos, fresh, ctl, ring):
    """One token of the particle stream's bookkeeping (cwlt_particle_advance): (pid or -1, tokens, done)
    of every row into row ctl[0] % R of ring (R, rows, A + 2) int64; pos += 1 for rows with pid >= 0; fresh = 0;
    ctl[0] += 1.  tokens (rows, A), pid / done / pos / fresh (rows,) int64; ctl int64, its element 0 the counter."""
    fn, rows, A = "particle_advance", pid.numel(), tokens.shape[-1]
    _int64_rows(fn, rows, pid=pid, done=done, pos=pos, fresh=fresh)
    _int64_rows(fn, rows * A, tokens=tokens)
    if ctl.dtype != torch.int64 or ctl.numel() < 1 or ring.dtype != torch.int64 or not ring.is_contiguous() or \
            ring.dim() != 3 or tuple(ring.shape[1:]) != (rows, A + 2):
        raise ValueError("%s: ctl int64 and ring a contiguous (R, %d, %d) int64" % (fn, rows, A + 2))
    _call("cwlt_particle_advance", _lib.dev(tokens, "tokens"), A, rows, _lib.dev(pid), _lib.dev(done), _lib.dev(pos),
          _lib.dev(fresh), _lib.dev(ctl), _lib.dev(ring), ring.shape[0], _lib.stream_ptr())


def _release_groups(fn, particles, n_songs, song, pid, pos, bar, cap, length, done, fresh, lw, log_z, out_lw, out_len,
                    out_logz, tables=()):
    """(groups, K) of a release, its state and output tensors checked in one pass (_int64_rows' check and message, one
    call for all sizes: the wrappers' Python time is the release's cost on the stream); tables: (name, tensor) pairs of
    (n_songs,) int64, the bank form's."""
    K, groups, N = int(particles), song.numel(), int(n_songs)
    rows = groups * K
    for name, t, n in (("song", song, groups), ("pid", pid, rows), ("pos", pos, rows), ("bar", bar, rows),
                       ("cap", cap, rows), ("length", length, rows), ("done", done, rows), ("fresh", fresh, rows),
                       ("out_len", out_len, N * K)) + tuple((name, t, N) for name, t in tables):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != n:
            raise TypeError(_INT64_ROWS % (fn, name, n))
    for t, n in ((lw, rows), (log_z, groups), (out_lw, N * K), (out_logz, N)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise TypeError("%s takes contiguous f32 lw (rows,), log_z (groups,), out_lw (n_songs * K,) and out_logz "
                            "(n_songs,)" % fn)
    return groups, K


def particle_release(particles, n_songs, bar0, cap0, song, pid, pos, bar, cap, length, done, fresh, lw, log_z, ctl,
                     out_lw, out_len, out_logz):
    """The release / hand-out of the particle stream (cwlt_particle_release; sampling.particle_release is
    its numpy restatement): groups without a song or with every row done are candidates; finished ones write out_lw,
    out_len (n_songs * particles,) and out_logz (n_songs,); candidates take the next songs from ctl[1] in group order.
    song, log_z (groups,); pid, pos, bar, cap, length, done, fresh, lw (rows,); ctl (>= 3,) int64."""
    fn = "particle_release"
    groups, K = _release_groups(fn, particles, n_songs, song, pid, pos, bar, cap, length, done, fresh, lw, log_z, out_lw,
                                out_len, out_logz)
    if ctl.dtype != torch.int64 or ctl.numel() < 3:
        raise TypeError("%s: ctl must hold the int64 counters {tokens, assigned, finished}" % fn)
    _call("cwlt_particle_release", groups, K, int(n_songs), int(bar0), int(cap0), _lib.dev(song), _lib.dev(pid),
          _lib.dev(pos), _lib.dev(bar), _lib.dev(cap), _lib.dev(length), _lib.dev(done), _lib.dev(fresh), _lib.dev(lw),
          _lib.dev(log_z), _lib.dev(ctl), _lib.dev(out_lw), _lib.dev(out_len), _lib.dev(out_logz), _lib.stream_ptr())


def particle_fill(dst, src, fresh, pid):
    """dst[n] = src[pid[n]] for the rows with fresh[n] != 0 and 0 <= pid[n] < len(src) (cwlt_particle_fill): the new
    particles' start rows.  dst (rows, ...) and src (n_src, ...) of one dtype and row width (4-byte multiples), unit
    stride inside a row; fresh, pid (rows,) int64."""
    fn, rows = "particle_fill", fresh.numel()
    _int64_rows(fn, rows, fresh=fresh, pid=pid)
    if dst.dtype != src.dtype or dst.shape[0] != rows or dst.dim() > 2 or src.dim() != dst.dim() or \
            dst.shape[1:] != src.shape[1:] or (dst.dim() == 2 and (dst.stride(1) != 1 or src.stride(1) != 1)):
        raise TypeError("%s takes dst (rows, w) and src (n_src, w) of one dtype, rows %d" % (fn, rows))
    es = dst.element_size()
    width = es * (dst.shape[1] if dst.dim() == 2 else 1)
    _call("cwlt_particle_fill", _lib.dev(dst, "dst"), _lib.dev(src, "src"), _lib.dev(fresh), _lib.dev(pid), rows,
          src.shape[0], width, es * dst.stride(0), es * src.stride(0), _lib.stream_ptr())
    return dst


def particle_refill_bank(state, bank_state, n_layer, s_floats, z_floats, logits, bank_logits, fresh, pid, particles):
    """The fresh rows of a particle pool take their song's bank entry (cwlt_particle_refill_bank): row n
    with fresh[n] and pid[n] >= 0 gets entry (pid[n] // particles) % bank, each float4 of an entry loaded once for the
    group's fresh rows.  state: flat f32 n_layer x [S (rows, s_floats), Z (rows, z_floats)]; bank_state the same for
    `bank` entries; logits (rows, >= n) and bank_logits (bank, n) f32; fresh, pid (rows,) int64."""
    fn, rows, per, K = "particle_refill_bank", fresh.numel(), s_floats + z_floats, int(particles)
    bank = bank_logits.shape[0]
    if state.dtype != torch.float32 or bank_state.dtype != torch.float32 or bank_logits.dtype != torch.float32 or \
            logits.dtype != torch.float32:
        raise TypeError("%s takes f32 state / logits" % fn)
    _int64_rows(fn, rows, fresh=fresh, pid=pid)
    if K < 1 or rows % K:
        raise ValueError("%s: %d rows are no whole groups of %d particles" % (fn, rows, K))
    if state.numel() != n_layer * rows * per or bank_state.numel() != n_layer * bank * per:
        raise ValueError("%s: state holds %d floats, bank %d, for %d layers x %d rows / %d entries x %d"
                         % (fn, state.numel(), bank_state.numel(), n_layer, rows, bank, per))
    if logits.shape[0] != rows or logits.stride(-1) != 1 or bank_logits.stride(-1) != 1 or \
            bank_logits.shape[1] > logits.shape[1]:
        raise ValueError("%s: logits must be (rows, >= n_logits), bank_logits (bank, n_logits), unit column strides"
                         % fn)
    _call("cwlt_particle_refill_bank", _lib.dev(state, "state"), _lib.dev(bank_state, "bank_state"), bank, int(n_layer),
          int(s_floats), int(z_floats), _lib.dev(logits, "logits"), _lib.dev(bank_logits, "bank_logits"),
          bank_logits.shape[1], logits.stride(0), bank_logits.stride(0), _lib.dev(fresh, "fresh"), _lib.dev(pid, "pid"),
          rows, K, _lib.stream_ptr())


def particle_release_bank(particles, n_songs, bar0_all, cap_all, song, pid, pos, bar, cap, length, done, fresh, lw,
                          log_z, ctl, out_lw, out_len, out_logz):
    """particle_release gated by the songs the bank has ready, each song with its own start (cwlt_particle_release_bank,
    DESIGN §4.6q; sampling.particle_release_bank restates the decision): songs are handed out only below
    min(ctl[3], n_songs), a candidate past that is parked until the next boundary, and a row handed song v starts from
    bar0_all[v] and cap_all[v] ((n_songs,) int64).  ctl (4,) int64 {tokens, assigned, finished, ready}."""
    fn = "particle_release_bank"
    groups, K = _release_groups(fn, particles, n_songs, song, pid, pos, bar, cap, length, done, fresh, lw, log_z, out_lw,
                                out_len, out_logz, (("bar0_all", bar0_all), ("cap_all", cap_all)))
    if ctl.dtype != torch.int64 or not ctl.is_contiguous() or ctl.numel() < 4:
        raise TypeError("%s: ctl must hold the int64 counters {tokens, assigned, finished, ready}" % fn)
    _call("cwlt_particle_release_bank", groups, K, int(n_songs), _lib.dev(bar0_all), _lib.dev(cap_all), _lib.dev(song),
          _lib.dev(pid), _lib.dev(pos), _lib.dev(bar), _lib.dev(cap), _lib.dev(length), _lib.dev(done), _lib.dev(fresh),
          _lib.dev(lw), _lib.dev(log_z), _lib.dev(ctl), _lib.dev(out_lw), _lib.dev(out_len), _lib.dev(out_logz),
          _lib.stream_ptr())


def _reward_ring(where, recent, live):
    """(rows, W, A) of a reward ring: recent (rows, W, A) and live (rows, W), contiguous int64."""
    if recent.dtype != torch.int64 or live.dtype != torch.int64 or not recent.is_contiguous() or not live.is_contiguous():
        raise TypeError("%s takes contiguous int64 recent and live" % where)
    if recent.dim() != 3 or tuple(live.shape) != tuple(recent.shape[:2]):
        raise ValueError("%s: recent must be (rows, W, A) and live (rows, W), got %s and %s"
                         % (where, tuple(recent.shape), tuple(live.shape)))
    return tuple(recent.shape)


def reward_push(tok, done, counter, recent, live):
    """One token into the particles' reward windows (cwlt_reward_push): with s = *counter % W,
    recent[n, s] = tok[n] and live[n, s] = (done[n] == 0).  tok (rows, A) int64, the token just drawn; done (rows,)
    int64 as it was BEFORE this token (call ahead of particle_weigh); counter the loop's device int64 row counter;
    recent (rows, W, A), live (rows, W) int64."""
    rows, W, A = _reward_ring("reward_push", recent, live)
    for t, n in ((tok, rows * A), (done, rows)):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != n:
            raise TypeError("reward_push takes contiguous int64 tok (%d, %d) and done (%d,)" % (rows, A, rows))
    if counter.dtype != torch.int64 or counter.numel() != 1:
        raise TypeError("reward_push: counter must be one device int64")
    _call("cwlt_reward_push", _lib.dev(tok, "tok"), _lib.dev(done, "done"), _lib.dev(counter, "counter"), rows, A, W,
          _lib.dev(recent, "recent"), _lib.dev(live, "live"), _lib.stream_ptr())


def reward_window(recent, live, filled, win, mask, any_live):
    """The particles' windows as a reward callable sees them (cwlt_reward_window): slots 0 .. filled - 1
    of the rings hold the window's rows in time order.  win[n, j] = recent[n, j] and mask[n, j] = 1 where j < filled and
    live[n, j], else token 0 and mask 0; any_live[n] = whether row n has such a slot; a row with none gets
    mask[n, 0] = 1.  win (rows, W, A), mask (rows, W), any_live (rows,) int64."""
    rows, W, A = _reward_ring("reward_window", recent, live)
    for t, shape in ((win, (rows, W, A)), (mask, (rows, W)), (any_live, (rows,))):
        if t.dtype != torch.int64 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise TypeError("reward_window takes contiguous int64 win (rows, W, A), mask (rows, W) and any (rows,)")
    _call("cwlt_reward_window", _lib.dev(recent, "recent"), _lib.dev(live, "live"), rows, A, W, int(filled),
          _lib.dev(win, "win"), _lib.dev(mask, "mask"), _lib.dev(any_live, "any"), _lib.stream_ptr())
    return win, mask, any_live


def _reward_rows(fn, r, any_live, lw, h_r):
    """The rows of a reward_apply: r, lw, h_r contiguous f32 and any_live contiguous int64, all of lw's length."""
    rows = lw.numel()
    for t in (r, lw, h_r):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != rows:
            raise TypeError("%s takes contiguous f32 r, lw and h_r of %d rows" % (fn, rows))
    if any_live.dtype != torch.int64 or not any_live.is_contiguous() or any_live.numel() != rows:
        raise TypeError("%s takes a contiguous int64 any of %d rows" % (fn, rows))
    return rows


def reward_apply(r, any_live, beta, lw, h_r):
    """The window rewards into the log-weights (cwlt_reward_apply): rows with any_live[n] != 0 get
    lw[n] = lw[n] + (beta * r[n]) (two f32 roundings, bitwise sampling.reward_apply_f32) and h_r[n] = r[n]; the others
    keep lw and get h_r[n] = 0, whatever r[n] holds.  r, lw, h_r (rows,) f32, any_live (rows,) int64."""
    rows = _reward_rows("reward_apply", r, any_live, lw, h_r)
    _call("cwlt_reward_apply", _lib.dev(r, "r"), _lib.dev(any_live, "any"), float(beta), rows, _lib.dev(lw, "lw"),
          _lib.dev(h_r, "h_r"), _lib.stream_ptr())
    return lw


def reward_apply_keyed(r, any_live, beta, key, particles, lw, h_r):
    """reward_apply with a reward weight per song (cwlt_reward_apply_keyed): row n is a row of song
    s = id // particles, id = key[n] (key None: n, the lock-step pool's rows).  Rows with any_live[n] != 0, id >= 0 and
    s < len(beta) get lw[n] = lw[n] + (beta[s] * r[n]) (two f32 roundings, bitwise sampling.reward_apply_keyed_f32) and
    h_r[n] = r[n]; the others keep lw and get h_r[n] = 0, whatever r[n] holds.  r, lw, h_r (rows,) f32, any_live (rows,)
    int64, beta (n_beta,) f32 on the device, key (rows,) int64 or None."""
    rows = _reward_rows("reward_apply_keyed", r, any_live, lw, h_r)
    if beta.dtype != torch.float32 or not beta.is_contiguous() or beta.dim() != 1 or beta.numel() < 1:
        raise TypeError("reward_apply_keyed takes a contiguous (n_beta,) f32 beta table")
    if key is not None and (key.dtype != torch.int64 or not key.is_contiguous() or key.numel() != rows):
        raise TypeError("reward_apply_keyed takes a contiguous int64 key of %d rows, or None" % rows)
    if int(particles) < 1:
        raise ValueError("reward_apply_keyed: particles must be >= 1, got %r" % (particles,))
    _call("cwlt_reward_apply_keyed", _lib.dev(r, "r"), _lib.dev(any_live, "any"), _lib.dev(beta, "beta"), beta.numel(),
          _lib.opt(key, "key"), int(particles), rows, _lib.dev(lw, "lw"), _lib.dev(h_r, "h_r"), _lib.stream_ptr())
    return lw


def song_metrics(tok, mask, lengths, attrs, order, pitch, chord, Q, xlog2x, max_bars, feat, weights=None, reward=None,
                 bars=None, hist=None, groove=None):
    """The 11 song measures of metrics.METRICS per song (cwlt_song_metrics; bitwise
    sampling.song_metrics_f32), one launch on the current stream, no sync.  tok (N, L, A) int64; mask (N, L) int64 or
    None; lengths (N,) int32 or None; attrs = (bar_attr, pitch_attr, chord_attr) column indices, chord_attr -1 (then
    chord may be None) for no chord feature; order / pitch / chord int32 tables and xlog2x (>= L + 1,) f32 as
    metrics.SongMetricSpec builds them.  Written: feat (N, 11) f32; with weights (11,) f32, reward (N,) f32; bars (N,)
    int32, hist (N, max_bars, 12) int32 and groove (N, max_bars) int64 where given."""
    if tok.dtype != torch.int64 or not tok.is_contiguous() or tok.dim() != 3:
        raise TypeError("song_metrics takes a contiguous int64 tok (N, L, A)")
    N, L, A = tok.shape
    MB = int(max_bars)
    if mask is not None and (mask.dtype != torch.int64 or not mask.is_contiguous() or tuple(mask.shape) != (N, L)):
        raise TypeError("song_metrics takes a contiguous int64 mask (%d, %d), or None" % (N, L))
    if lengths is not None and (lengths.dtype != torch.int32 or not lengths.is_contiguous()
                                or tuple(lengths.shape) != (N,)):
        raise TypeError("song_metrics takes contiguous int32 lengths (%d,), or None" % N)
    for t, name in ((order, "order"), (pitch, "pitch"), (chord, "chord")):
        if t is None and name == "chord":
            continue
        if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1:
            raise TypeError("song_metrics takes a contiguous int32 %s table" % name)
    for t, shape, name in ((xlog2x, None, "xlog2x"), (feat, (N, 11), "feat"), (weights, (11,), "weights"),
                           (reward, (N,), "reward")):
        if t is None and name in ("weights", "reward"):
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise TypeError("song_metrics takes a contiguous f32 %s%s" % (name, "" if shape is None else " %s" % (shape,)))
    for t, dt, shape, name in ((bars, torch.int32, (N,), "bars"), (hist, torch.int32, (N, MB, 12), "hist"),
                               (groove, torch.int64, (N, MB), "groove")):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape):
            raise TypeError("song_metrics takes a contiguous %s %s %s, or None" % (dt, name, shape))
    bar_attr, pitch_attr, chord_attr = (int(x) for x in attrs)
    _call("cwlt_song_metrics", _lib.dev(tok, "tok"), _lib.opt(mask, "mask"), _lib.opt(lengths, "lengths"), N, L, A,
          bar_attr, pitch_attr, chord_attr, _lib.dev(order, "order"), order.numel(), _lib.dev(pitch, "pitch"),
          pitch.numel(), _lib.opt(chord, "chord"), 0 if chord is None else chord.numel(), int(Q),
          _lib.dev(xlog2x, "xlog2x"), xlog2x.numel(), MB, _lib.dev(feat, "feat"), _lib.opt(weights, "weights"),
          _lib.opt(reward, "reward"), _lib.opt(bars, "bars"), _lib.opt(hist, "hist"), _lib.opt(groove, "groove"),
          _lib.stream_ptr())
    return feat


def stream_refill(state, snap_state, n_layer, s_floats, z_floats, logits, snap_logits, fresh):
    """Copy the one-slot snapshot (state, logits) into every slot whose fresh flag is set (cwlt_stream_refill).
    state: flat f32 of n_layer x [S (slots, s_floats), Z (slots, z_floats)] (DecodeSession._state); snap_state: the same
    for one slot; logits (slots, >= n) f32 with snap_logits (n,) f32; fresh (slots,) int64."""
    slots = fresh.numel()
    per = s_floats + z_floats
    if state.dtype != torch.float32 or snap_state.dtype != torch.float32 or fresh.dtype != torch.int64:
        raise TypeError("stream_refill takes f32 state / logits and int64 flags")
    if state.numel() != n_layer * slots * per or snap_state.numel() != n_layer * per:
        raise ValueError("stream_refill: state holds %d floats, snapshot %d, for %d layers x %d slots x %d"
                         % (state.numel(), snap_state.numel(), n_layer, slots, per))
    if logits.shape[0] != slots or logits.stride(-1) != 1 or snap_logits.numel() > logits.shape[1]:
        raise ValueError("stream_refill: logits must be (slots, >= n_logits) with unit column stride")
    _call("cwlt_stream_refill", _lib.dev(state, "state"), _lib.dev(snap_state.contiguous(), "snap_state"), int(n_layer),
          int(s_floats), int(z_floats), _lib.dev(logits, "logits"), _lib.dev(snap_logits.contiguous(), "snap_logits"),
          snap_logits.numel(), logits.stride(0), _lib.dev(fresh, "fresh"), slots, _lib.stream_ptr())


def stream_advance(tokens, bar_attr, bar_mask, bar_cond, bar0, cap, n_songs, song, pos, bar, fresh, ctl, ring):
    """One token of the stream's slot bookkeeping (cwlt_stream_advance): tokens (slots, A) int64 just drawn; bar_mask
    (n_class[bar_attr],) int32; song / pos / bar / fresh (slots,) int64; ctl (3,) int64; ring (R, slots, A + 2) int64."""
    slots, A = song.numel(), tokens.shape[-1]
    for t in (song, pos, bar, fresh, ctl, ring, tokens):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError("stream_advance takes contiguous int64 slot arrays")
    if bar_mask.dtype != torch.int32 or tokens.numel() != slots * A or ring.shape[1:] != (slots, A + 2) or \
            ctl.numel() != 3 or not all(t.numel() == slots for t in (pos, bar, fresh)):
        raise ValueError("stream_advance: inconsistent slot array shapes")
    _call("cwlt_stream_advance", _lib.dev(tokens, "tokens"), A, slots, int(bar_attr), _lib.dev(bar_mask, "bar_mask"),
          bar_mask.numel(), int(bar_cond), int(bar0), int(cap), int(n_songs), _lib.dev(song), _lib.dev(pos),
          _lib.dev(bar), _lib.dev(fresh), _lib.dev(ctl), _lib.dev(ring), ring.shape[0], _lib.stream_ptr())


def stream_refill_bank(state, bank_state, n_layer, s_floats, z_floats, logits, bank_logits, fresh, song):
    """Copy each fresh slot's start from the bank (cwlt_stream_refill_bank): slot s with fresh[s] and song[s] >= 0 gets
    entry song[s] % bank.  state: flat f32 n_layer x [S (slots, s_floats), Z (slots, z_floats)]; bank_state the same
    for `bank` entries; logits (slots, >= n) and bank_logits (bank, n) f32; fresh, song (slots,) int64."""
    slots, per = fresh.numel(), s_floats + z_floats
    bank = bank_logits.shape[0]
    if state.dtype != torch.float32 or bank_state.dtype != torch.float32 or bank_logits.dtype != torch.float32:
        raise TypeError("stream_refill_bank takes f32 state / logits")
    if fresh.dtype != torch.int64 or song.dtype != torch.int64 or song.numel() != slots:
        raise TypeError("stream_refill_bank takes (slots,) int64 fresh flags and songs")
    if state.numel() != n_layer * slots * per or bank_state.numel() != n_layer * bank * per:
        raise ValueError("stream_refill_bank: state holds %d floats, bank %d, for %d layers x %d slots / %d entries x %d"
                         % (state.numel(), bank_state.numel(), n_layer, slots, bank, per))
    if logits.shape[0] != slots or logits.stride(-1) != 1 or bank_logits.stride(-1) != 1 or \
            bank_logits.shape[1] > logits.shape[1]:
        raise ValueError("stream_refill_bank: logits must be (slots, >= n_logits), bank_logits (bank, n_logits), unit "
                         "column strides")
    _call("cwlt_stream_refill_bank", _lib.dev(state, "state"), _lib.dev(bank_state, "bank_state"), bank, int(n_layer),
          int(s_floats), int(z_floats), _lib.dev(logits, "logits"), _lib.dev(bank_logits, "bank_logits"),
          bank_logits.shape[1], logits.stride(0), bank_logits.stride(0), _lib.dev(fresh, "fresh"),
          _lib.dev(song, "song"), slots, _lib.stream_ptr())


def stream_advance_bank(tokens, bar_attr, bar_mask, bar_cond, bank_bar0, bank_cap, n_songs, song, pos, bar, cap, fresh,
                        ctl, ring):
    """stream_advance with per-song bar0 / cap from the bank and the ready gate (cwlt_stream_advance_bank): bank_bar0,
    bank_cap (bank,) int64; cap (slots,) int64 the slots' own caps; ctl (4,) int64 {tokens, assigned, finished, ready};
    a waiting slot holds song -2."""
    slots, A = song.numel(), tokens.shape[-1]
    for t in (song, pos, bar, cap, fresh, ctl, ring, tokens, bank_bar0, bank_cap):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError("stream_advance_bank takes contiguous int64 slot and bank arrays")
    if bar_mask.dtype != torch.int32 or tokens.numel() != slots * A or ring.shape[1:] != (slots, A + 2) or \
            ctl.numel() != 4 or not all(t.numel() == slots for t in (pos, bar, cap, fresh)) or \
            bank_cap.numel() != bank_bar0.numel():
        raise ValueError("stream_advance_bank: inconsistent slot or bank array shapes")
    _call("cwlt_stream_advance_bank", _lib.dev(tokens, "tokens"), A, slots, int(bar_attr),
          _lib.dev(bar_mask, "bar_mask"), bar_mask.numel(), int(bar_cond), _lib.dev(bank_bar0), _lib.dev(bank_cap),
          bank_bar0.numel(), int(n_songs), _lib.dev(song), _lib.dev(pos), _lib.dev(bar), _lib.dev(cap),
          _lib.dev(fresh), _lib.dev(ctl), _lib.dev(ring), ring.shape[0], _lib.stream_ptr())
