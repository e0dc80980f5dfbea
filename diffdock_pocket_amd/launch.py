"""Thin host wrappers around the C ABI of libddp_hip.so (include/ddp_hip.h) for the score-model forward: conv / reduce /
featurise / stage-A launches and the batched index-list primitives with device-side counts.

Every launch goes to the CURRENT stream of the CURRENT device (one C call to fetch the raw handle); the forward runs inside
`torch.cuda.device(batch device)`, so the searches, list kernels, convs and the pose update of one model share one stream
whatever the process-wide current device is.  Nothing here synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import nn

from . import _lib as L
from . import packing as P
from .graph import EdgeView


def require_hip(t: torch.Tensor):
    if not t.is_cuda:
        raise L.DdpError("the MI355X score model runs on a HIP device only (no CPU/eager fallback); "
                         "move the batch to cuda:<n>")
    L.load()


def stream():
    """Raw handle of the current HIP stream of the current device (torch.cuda.current_stream() is ~9 us of Python)."""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _p(t: Optional[torch.Tensor]) -> int:
    return t.data_ptr() if t is not None else 0


# ------------------------------------------------------------------------------------------------ device-side counts
class CountBlock:
    """The device-side sizes of one forward's pose-dependent lists: named int32 slots of one small tensor.  `cnt[name]` is a
    1-element view (allocated on first use) whose address goes to the kernels; nothing reads it on the host unless asked
    (`value`, used by last_stats / the profiler AFTER the step has been queued)."""

    SLOTS = 256

    def __init__(self, dev):
        self.block = torch.zeros(self.SLOTS, dtype=torch.int32, device=dev)
        self.index: Dict[str, int] = {}

    def __getitem__(self, name: str) -> torch.Tensor:
        i = self.index.get(name)
        if i is None:
            i = self.index[name] = len(self.index)
            if i >= self.SLOTS:
                raise L.DdpError("CountBlock: out of slots")
        return self.block[i:i + 1]

    def __contains__(self, name):
        return name in self.index

    def values(self) -> Dict[str, int]:
        """Host copy of every named slot (one device-to-host copy: a host synchronisation)."""
        host = self.block.tolist()
        return {k: int(host[i]) for k, i in self.index.items()}


# ------------------------------------------------------------------------------------------------ profiling hooks
class ConvProfiler:
    """Times every ddp_conv_messages launch with HIP events on the launch stream and tallies its algorithmic FLOPs
    (BASELINE.md section 3 formula x the launch's actual edge count).  Used by bench.py for the roofline entry.  Edge counts
    that live in device memory are resolved when a summary is asked for (after the timed region)."""

    def __init__(self):
        self.events, self.kernel, self.specs, self.counts, self.node_bytes, self.tags, self.h2 = [], [], [], [], [], [], []
        self.hbm = {}   # HBM-bound kernels: name -> [(event0, event1, bytes or callable)]
        self.hbm_on = False   # their ~45 extra event pairs per step cost wall time: bench.py times them in extra steps
        self._resolved = None

    # -- recording (called by the launch wrappers) -------------------------------------------------------------
    def record_conv(self, e0, e1, spec, flops_spec, tasks_counts, node_bytes, tag=None, h2=False, rows=False):
        """tasks_counts: [(capacity, cnt tensor or None)] of the launch's tasks; tag: where in the forward the launch sits
        ("layer3", "head")."""
        self.events.append((e0, e1))
        self.tags.append(tag)
        self.h2.append(bool(h2))     # the launch ran the fp16 hi/lo split form of the fc products
        # (rows: 1 = ddp_conv_rows_kernel, the v_mfma_f32_32x32x16_f16 form; 2 = ddp_conv_rows16_kernel, the 16x16x32 form)
        self.kernel.append((("ddp_conv_rows16_kernel" if spec.factorized else "ddp_conv_rows16_direct_kernel") if int(rows) == 2 else "ddp_conv_rows_kernel") if rows else
                           "ddp_conv32_kernel" if spec.factorized else "ddp_conv_messages_kernel")
        self.specs.append((spec, flops_spec or spec))
        self.counts.append(tasks_counts)
        self.node_bytes.append(node_bytes)
        self._resolved = None

    def _resolve(self):
        if self._resolved is None:
            torch.cuda.synchronize()
            cache = {}

            def val(cap, cnt):
                if cnt is None:
                    return cap
                key = (cnt.data_ptr(), id(cnt))
                if key not in cache:
                    cache[key] = min(cap, max(0, int(cnt.item())))
                return cache[key]

            ne = [sum(val(c, t) for c, t in tc) for tc in self.counts]
            self.edges = ne
            self.flops = [fs.flops_per_edge() * n for (s, fs), n in zip(self.specs, ne)]
            self.executed = [(s.mfma_flops_per_edge_executed() + 2 * s.hid * sum(s.g_cols)) * n for (s, fs), n in zip(self.specs, ne)]
            self.useful = [s.useful_flops_per_edge() * n for (s, fs), n in zip(self.specs, ne)]
            # product FLOPs that run as fp16 hi/lo split products: the two fc products; ddp_conv_rows also runs the per-edge G contraction
            # (h @ G[src]: 2 hid g_cols per edge) as tile products of the same form
            self.fc = [(s.fc_flops_per_edge() + (2 * s.hid * sum(s.g_cols) if k.startswith("ddp_conv_rows") else 0)) * n
                       for (s, fs), n, k in zip(self.specs, ne, self.kernel)]
            self.boundary = [n * (4.0 * fs.f_in + 32.0) + nb for (s, fs), n, nb in zip(self.specs, ne, self.node_bytes)]
            self._resolved = True

    # -- summaries ------------------------------------------------------------------------------------------------
    def hbm_summary(self, name):
        """(launches, algorithmic bytes, ms) of an HBM-bound kernel (ddp_stage_a_mfma_kernel, ddp_segment_reduce_kernel)."""
        rec = self.hbm.get(name, [])
        torch.cuda.synchronize()
        return len(rec), float(sum((r[2]() if callable(r[2]) else r[2]) for r in rec)), float(sum(r[0].elapsed_time(r[1]) for r in rec))

    def summary(self, kernel=None):
        """(launches, algorithmic FLOPs, ms) over all launches or over those of one kernel instantiation
        ("ddp_conv32_kernel": factorised shapes, "ddp_conv_messages_kernel": direct shapes)."""
        self._resolve()
        sel = [i for i, k in enumerate(self.kernel) if kernel is None or k == kernel]
        ms = sum(self.events[i][0].elapsed_time(self.events[i][1]) for i in sel)
        return len(sel), float(sum(self.flops[i] for i in sel)), float(ms)

    def split_flops(self, kernel=None, tag=False):
        """(fc-product FLOPs of the launches that ran the h2 form, all other useful FLOPs) of one kernel instantiation: the first run
        on the fp16 matrix cores at three instruction FLOPs per product FLOP, the rest (fp32-MFMA launches, G pass, contraction) in
        fp32."""
        self._resolve()
        fc16 = sum(f for f, k, h in zip(self.fc, self.kernel, self.h2) if h and (kernel is None or k == kernel))
        useful = sum(u for u, k in zip(self.useful, self.kernel) if kernel is None or k == kernel)
        return float(fc16), float(useful - fc16)

    def by_tag(self, kernel):
        """{tag: (launches, useful FLOPs, ms, edges, fc FLOPs run in the h2 form)} of one kernel instantiation, e.g. per conv layer."""
        self._resolve()
        out = {}
        for i, k in enumerate(self.kernel):
            if k != kernel:
                continue
            n, u, ms, ne, f16 = out.get(self.tags[i], (0, 0.0, 0.0, 0, 0.0))
            out[self.tags[i]] = (n + 1, u + self.useful[i], ms + self.events[i][0].elapsed_time(self.events[i][1]), ne + self.edges[i],
                                 f16 + (self.fc[i] if self.h2[i] else 0.0))
        return out

    def executed_flops(self, kernel=None):
        """FLOPs of the padded MFMA tiles + the G pass of factorised convs (a model of what is issued; the PMC pass counts it)."""
        self._resolve()
        return float(sum(e for e, k in zip(self.executed, self.kernel) if kernel is None or k == kernel))

    def useful_flops(self, kernel=None):
        """Useful fp32 FLOPs of the executed formulation without padding (packing.ConvSpec.useful_flops_per_edge)."""
        self._resolve()
        return float(sum(e for e, k in zip(self.useful, self.kernel) if kernel is None or k == kernel))

    def boundary_bytes(self):
        """Algorithmic bytes at the module boundary of the recorded conv calls (SURVEY section 8(d):
        4 (N_in D_in + E F + 4 E + N_out D_out) + 16 E per TensorProductConvLayer.forward call)."""
        self._resolve()
        return float(sum(self.boundary))


_PROFILER: Optional[ConvProfiler] = None


def set_conv_profiler(p: Optional[ConvProfiler]):
    global _PROFILER
    _PROFILER = p


def profiler(hbm=False) -> Optional[ConvProfiler]:
    p = _PROFILER
    if p is not None and hbm and not p.hbm_on:
        return None
    return p


class SectionTimer:
    """Diagnostic: `model.section_timer = SectionTimer()` records a device event and the host clock at each section
    boundary of forward; `summary()` gives per-section (gpu_ms, host_ms) summed over the recorded calls."""

    def __init__(self):
        self.marks = []

    def mark(self, name):
        import time
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append((name, ev, time.perf_counter()))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for (n0, e0, t0), (n1, e1, t1) in zip(self.marks[:-1], self.marks[1:]):
            if n1 == "start":
                continue
            g, h = out.get(n1, (0.0, 0.0))
            out[n1] = (g + e0.elapsed_time(e1), h + (t1 - t0) * 1e3)
        return out


# ------------------------------------------------------------------------------------------------ conv / reduce
# The fc products of the conv kernels on the fp16 matrix cores with both operands split in two halves (three products per 16 k,
# fp32 accumulation; csrc/ddp_conv.hip).  False: the exact fp32 MFMA chains of rounds 1 - 3 (A/B runs, the h2-vs-fp32 tests).
CONV_H2 = True
# where the h2 kernels report a value outside the fp16 range: an int32 in pinned host memory (score_model.overflow_flag(dev)[1:2]),
# set by the forward that is being queued (engine.forward); None: not reported
_RANGE_FLAG = None


def set_range_flag(t):
    global _RANGE_FLAG
    _RANGE_FLAG = t


# Factorised convs of the size classes ns = 60 / 32 through the 128-edge row-stationary kernel (ddp_conv_rows, csrc/ddp_conv_rows.hip; needs
# CONV_H2).  False: the 32-edge kernel of rounds 2 - 4 (A/B runs).  The two read G in different layouts: a task carries one of them.
CONV_ROWS = os.environ.get("DDP_CONV_ROWS", "1") != "0"     # (environment: same-box A/B runs)


def occupancy_shaping(rows_min_lds: int = 0, stage_a_pad: int = 0):
    """ddp_set_occupancy_shaping (include/ddp_hip.h): launches enqueued from here on - ddp_conv_rows with at least `rows_min_lds` bytes of
    dynamic LDS (> 80 KiB: one workgroup per CU), stage A's plane form with `stage_a_pad` extra bytes.  (0, 0): the kernels' own."""
    L.check(L.load().ddp_set_occupancy_shaping(int(rows_min_lds), int(stage_a_pad)), "ddp_set_occupancy_shaping")


class ConvPath(NamedTuple):
    """How one conv task runs (conv_path): the kernel, the form of its fc products and, for ddp_conv_rows, the ddp_conv_task_t fields
    that select the kernel's form (include/ddp_hip.h).  Every task of one launch_convs call shares `rows` and `rows_form`."""
    rows: bool                  # ddp_conv_rows (else ddp_conv_messages); G then comes from stage A in plane form
    h2: bool                    # the fc products as fp16 hi/lo split products (w1h / w2h), else the exact fp32 MFMA form
    rows_form: int = 0          # operand images: 0 = v_mfma_f32_32x32x16_f16, 1 = v_mfma_f32_16x16x32_f16
    gh_fmt: int = 0             # plane form of G (factorised convs)
    rows_bias_k: int = 0        # the fc.3 bias in the padding k row (direct convs)
    rows_seg: tuple = (0, 0)    # the output-segment range of a direct conv's task; (0, 0): all
    rows_nts: int = 0           # stream tiles of that range


def conv_path(pk, rows_ok: bool = True) -> ConvPath:
    """The one place that decides how a conv task built from the packed weights `pk` runs, from the switches as they are when it is
    called: CONV_H2, CONV_ROWS and the caller's `rows_ok` (a model's all-or-none verdict, score_model.rows_all_or_none).  ddp_conv_rows
    where the pack carries its weight stream, ddp_conv_messages otherwise.  Stage A writes G in the layout of the same record."""
    h2 = CONV_H2 and pk.w1h is not None and pk.w2h is not None
    if not (CONV_H2 and CONV_ROWS and rows_ok and pk.wsh is not None):
        return ConvPath(False, h2)
    return ConvPath(True, h2, pk.rows_form, pk.gh_fmt, pk.rows_bias_k, pk.rows_seg, pk.rows_nts)


def make_task(pk, path: ConvPath, x_src, ldx_src, view: EdgeView, sh, segs, msg, g=None) -> L.ConvTask:
    """segs: [(tensor, idx_int32[E], ld, ncols)], concatenated into edge_attr_ in this order.  path: conv_path of `pk`; for ddp_conv_rows
    `g` holds the G arrays in plane form (ddp_stage_a_gh)."""
    t = L.ConvTask()
    t.x_src, t.ldx_src, t.n_edges = x_src.data_ptr(), ldx_src, view.n_edges
    t.src, t.eid, t.sh = view.src.data_ptr(), view.eid.data_ptr(), sh.data_ptr()
    for k in range(L.DDP_MAX_SEGS):
        if k < len(segs):
            ten, idx, ld, n = segs[k]
            t.seg_ptr[k], t.seg_idx[k], t.seg_ld[k], t.seg_n[k] = ten.data_ptr(), idx.data_ptr(), ld, n
        else:
            t.seg_ptr[k], t.seg_idx[k], t.seg_ld[k], t.seg_n[k] = 0, 0, 0, 0
    t.w1p, t.b1p, t.w2p, t.b2p = pk.w1p.data_ptr(), pk.b1p.data_ptr(), pk.w2p.data_ptr(), pk.b2p.data_ptr()
    t.w1h, t.w2h = (pk.w1h.data_ptr(), pk.w2h.data_ptr()) if path.h2 else (0, 0)
    t.h2_range_flag = _p(_RANGE_FLAG) if path.h2 else 0
    t.msg = msg.data_ptr()
    t.wsh, t.bsp = (pk.wsh.data_ptr(), pk.bsp.data_ptr()) if path.rows else (0, 0)
    for k in range(2):
        gk = g[k].data_ptr() if (g is not None and g[k] is not None) else 0
        t.g[k], t.gh[k] = (0, gk) if path.rows else (gk, 0)
    t.gh_fmt, t.rows_form, t.rows_bias_k, t.rows_nts = path.gh_fmt, path.rows_form, path.rows_bias_k, path.rows_nts
    t.rows_seg0, t.rows_seg1 = path.rows_seg
    t._path = path
    t.pos = _p(view.pos)
    t.n_edges_dev = _p(view.cnt)
    t._count = (view.n_edges, view.cnt)      # (python-side only: for the profiler)
    return t


def launch_convs(spec: P.ConvSpec, tasks: List[L.ConvTask], flops_spec: Optional[P.ConvSpec] = None, node_bytes: float = 0.0, tag=None):
    """One launch of the kernel the tasks' common path names (tasks that name different kernels are a caller's error).  node_bytes:
    4 (N_in D_in + N_out D_out) summed over the launch's conv calls; tag: position in the forward (both only used by the profiler)."""
    lib = L.load()
    if not tasks:
        return
    path = tasks[0]._path
    if any((t._path.rows, t._path.rows_form) != (path.rows, path.rows_form) for t in tasks):
        raise L.DdpError("launch_convs: the tasks of one launch run through different conv kernels")
    arr = (L.ConvTask * len(tasks))(*tasks)
    shape = spec.ctypes_shape()
    prof = _PROFILER
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if path.rows:
        L.check(lib.ddp_conv_rows(C.byref(shape), arr, len(tasks), stream()), "ddp_conv_rows")
    else:
        L.check(lib.ddp_conv_messages(C.byref(shape), arr, len(tasks), stream()), "ddp_conv_messages")
    if prof is not None:
        e1.record()
        h2 = P.h2_steps(spec) > 0 and all(t._path.h2 for t in tasks)
        prof.record_conv(e0, e1, spec, flops_spec, [t._count for t in tasks], node_bytes, tag, h2,
                         rows=(2 if path.rows_form == 1 else 1) if path.rows else 0)


def launch_reduce(x, ldx, n_nodes, d_out, sources, accumulate=True, n_rep=1, rep_stride=0):
    """sources: [(msg, view, packed[, rowmap])] in the reference's summation order; rowmap (int32 per CSR position, optional)
    = the row of `msg` that holds the position's message.  n_rep > 1: see ddp_segment_reduce."""
    lib = L.load()
    arr = (L.ReduceSrc * max(len(sources), 1))()
    for i, src_ in enumerate(sources):
        msg, view, pk = src_[:3]
        arr[i].msg, arr[i].rowptr = msg.data_ptr(), view.rowptr.data_ptr()
        arr[i].bn_scale, arr[i].bn_shift, arr[i].n_edges = pk.bn_scale.data_ptr(), pk.bn_shift.data_ptr(), view.n_edges
        arr[i].rowmap = src_[3].data_ptr() if (len(src_) > 3 and src_[3] is not None) else 0
        arr[i].n_edges_dev = _p(view.cnt)
    prof = profiler(hbm=True)
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.check(lib.ddp_segment_reduce(ptr(x), ldx, n_nodes, d_out, arr, len(sources), 1 if accumulate else 0, n_rep, rep_stride,
                                   stream()), "ddp_segment_reduce")
    if prof is not None:
        e1.record()
        # algorithmic bytes: every message row read once, every node row read and written once
        views = [s_[1] for s_ in sources]

        def nbytes(views=views, d_out=d_out, n_nodes=n_nodes, n_rep=n_rep):
            ne = sum(v.n_edges if v.cnt is None else min(v.n_edges, int(v.cnt.item())) for v in views)
            return 4.0 * d_out * (ne + 2 * n_nodes * max(n_rep, 1))
        # (the same predicate as csrc/ddp_misc.hip: the 16-byte form needs 16-byte aligned arrays and d_out, ldx multiples of 4)
        wide = (d_out % 4 == 0 and ldx % 4 == 0 and x.data_ptr() % 16 == 0 and not os.environ.get("DDP_REDUCE_NARROW")
                and all(s_[0].data_ptr() % 16 == 0 and s_[2].bn_scale.data_ptr() % 16 == 0 and s_[2].bn_shift.data_ptr() % 16 == 0 for s_ in sources))
        prof.hbm.setdefault("ddp_segment_reduce4_kernel" if wide else "ddp_segment_reduce_kernel", []).append((e0, e1, nbytes))


class EdgeMLPPack:
    """Host-side split of an edge-embedding MLP `Linear(in, ns) -> ReLU -> Linear(ns, ns)` for ddp_edge_featurize:
    the RBF columns of the first Linear go to the kernel (zero padded to 64 outputs); the other input columns
    (sigma embedding, bond type) plus the bias become the per-node / per-edge `pre` table."""

    def __init__(self, seq: nn.Sequential, rbf_slice: slice, device):
        W1, b1, W2, b2 = seq[0].weight.detach(), seq[0].bias.detach(), seq[3].weight.detach(), seq[3].bias.detach()
        ns = W1.shape[0]
        k = rbf_slice.stop - rbf_slice.start
        w1d = torch.zeros(k, 64, device=device)
        w1d[:, :ns] = W1[:, rbf_slice].t()
        w2 = torch.zeros(64, 64, device=device)
        w2[:ns, :ns] = W2.t()
        b2p = torch.zeros(64, device=device)
        b2p[:ns] = b2
        self.w1d, self.w2, self.b2, self.ns, self.k = w1d.contiguous(), w2.contiguous(), b2p, ns, k
        self.W1, self.b1 = W1, b1


def edge_featurize(pack: EdgeMLPPack, dist, pos_a, ia, pos_b, ib, pre, pre_idx, pre2=None, n_edges=None, cnt=None):
    """pre: [*, >= ns] rows with unit column stride (a column slice of a wider table is fine); pre2 (optional, [n2, ns]) is
    added to the first n2 edges' rows (the bond-type columns of lig_edge_embedding's first Linear).  n_edges / cnt: capacity
    and device-side count of the edge arrays (default: their length, host-known)."""
    lib = L.load()
    E = int(ia.shape[0]) if n_edges is None else int(n_edges)
    dev = pos_a.device
    out = torch.empty((E, pack.ns), device=dev, dtype=torch.float32)
    sh = torch.empty((E, 4), device=dev, dtype=torch.float32)
    if E == 0:
        return out, sh
    if pre.stride(1) != 1:
        pre = pre.contiguous()
    n2 = 0 if pre2 is None else int(pre2.shape[0])
    L.check(lib.ddp_edge_featurize(ptr(pos_a), ptr(ia), ptr(pos_b), ptr(ib), E, ptr(cnt), ptr(dist.offset), pack.k,
                                   C.c_float(dist.coeff), ptr(pre), ptr(pre_idx), pre.stride(0),
                                   ptr(pre2) if n2 else None, n2, pre2.stride(0) if n2 else 0, ptr(pack.w1d),
                                   ptr(pack.w2), ptr(pack.b2), pack.ns, ptr(out), ptr(sh), stream()),
            "ddp_edge_featurize")
    return out, sh


def edge_featurize_jobs(calls):
    """Several edge_featurize calls as ONE launch (ddp_edge_featurize_jobs).  calls: [(args, kwargs)] of `edge_featurize`;
    returns [(out, sh)].  Falls back to one launch per call when an MLP is outside the batched kernel's shape range."""
    if any(a[0].k % 8 or not 8 <= a[0].k <= 64 for a, _ in calls) or len(calls) > L.DDP_MAX_FEATURIZE_JOBS:
        return [edge_featurize(*a, **kw) for a, kw in calls]
    jobs, outs, keep = [], [], []
    for (pack, dist, pos_a, ia, pos_b, ib, pre, pre_idx), kw in calls:
        pre2, n_edges, cnt = kw.get("pre2"), kw.get("n_edges"), kw.get("cnt")
        E = int(ia.shape[0]) if n_edges is None else int(n_edges)
        out = torch.empty((E, pack.ns), device=pos_a.device, dtype=torch.float32)
        sh = torch.empty((E, 4), device=pos_a.device, dtype=torch.float32)
        outs.append((out, sh))
        if E == 0:
            continue
        if pre.stride(1) != 1:
            pre = pre.contiguous()
        n2 = 0 if pre2 is None else int(pre2.shape[0])
        j = L.FeaturizeJob()
        j.pos_a, j.ia, j.pos_b, j.ib, j.n_edges, j.n_edges_dev = _p(pos_a), _p(ia), _p(pos_b), _p(ib), E, _p(cnt)
        j.offset, j.k_rbf, j.coeff = _p(dist.offset), pack.k, float(dist.coeff)
        j.pre, j.pre_idx, j.ld_pre = _p(pre), _p(pre_idx), pre.stride(0)
        j.pre2, j.n_pre2, j.ld_pre2 = (_p(pre2) if n2 else 0), n2, (pre2.stride(0) if n2 else 0)
        j.w1d, j.w2, j.b2, j.ns, j.out, j.sh = _p(pack.w1d), _p(pack.w2), _p(pack.b2), pack.ns, _p(out), _p(sh)
        jobs.append(j)
        keep.append((pre, pre2, ia, ib, pre_idx))
    if jobs:
        arr = (L.FeaturizeJob * len(jobs))(*jobs)
        L.check(L.load().ddp_edge_featurize_jobs(arr, len(jobs), stream()), "ddp_edge_featurize_jobs")
    return outs


@dataclass
class StageAStack:
    """The stacked stage-A right-hand sides of factorised convs that read one source array: ONE launch computes every product
    (stage_a_stack builds it, stage_a launches it) - G in the plane form ddp_conv_rows reads (path.rows) or as fp32 rows."""
    W: torch.Tensor             # [nb, K, ncols] fp32
    meta: list                  # per product: (key, G slot, first input column)
    offs: object                # the first input columns as a ctypes int32 array
    path: ConvPath              # of the convs: G leaves in its layout
    gh: Optional[torch.Tensor]  # destination table of the plane form (packing.gh_dest_table), path.rows only
    ld: int                     # floats per output row (plane form 1: 3 / 4 of the product's columns)
    Wh: Optional[torch.Tensor] = None       # W split for the fp16 hi/lo form (packing.split_h2)
    W3: Optional[torch.Tensor] = None       # W split for the bf16x3 form (packing.split_bf16x3)

    def prepare(self, h2: bool, x3: bool) -> "StageAStack":
        """Makes the split weights a launch with these options reads (once: the options may change between two forwards)."""
        if (h2 or self.path.rows) and self.Wh is None:
            self.Wh = P.split_h2(self.W, unified_scale=P.GH_SW) if self.path.rows else P.split_h2(self.W)
        if x3 and not self.path.rows and self.W3 is None:
            self.W3 = P.split_bf16x3(self.W)
        return self


def stage_a_stack(packs, hid: int, path: ConvPath) -> StageAStack:
    """packs: [(key, packed weights)] of convs that read the same source rows and run by `path` (conv_path): their G arrays in the
    layout the conv tasks read."""
    Ws, meta, ghs, lds = [], [], [], set()
    for key, pk in packs:
        for slot in (0, 1):
            if pk.wg[slot] is None:
                continue
            meta.append((key, slot, pk.g_in_off[slot]))
            Ws.append(pk.wgh[slot] if path.rows else pk.wg[slot])
            if path.rows:
                ghs.append(pk.gh_groups[slot])
                lds.add(pk.gh_ld[slot])
    assert len(lds) <= 1, "the convs of one stage-A launch write G rows of one length"
    W = torch.stack(Ws).contiguous()
    gh = torch.stack([P.gh_dest_table(ws, (hid + 7) // 8, W.shape[2], fmt=path.gh_fmt) for ws in ghs]).contiguous().to(W.device) if path.rows else None
    return StageAStack(W, meta, (C.c_int32 * len(meta))(*[mm[2] for mm in meta]), path, gh, lds.pop() if lds else W.shape[2])


def stage_a(x, n_rows, st: StageAStack, out, rows=None, rows_cnt=None, out_rows=None, h2=False, x3=False):
    """ddp_stage_a: out[b][row] = x[row, offs[b]:offs[b]+k] @ W[b] for the listed rows (all n_rows rows if rows is None) and every
    product b of the stack.  st.path.rows: the output leaves in the layout ddp_conv_rows reads (ddp_stage_a_gh / _gh3); otherwise h2: the
    fp16 hi/lo form (ddp_stage_a_h2), x3: the bf16x3 form, neither: exact fp32 MFMA.  (st.prepare(h2, x3) first.)"""
    lib = L.load()
    nb, n_in, ncols = st.W.shape
    if nb > L.DDP_MAX_GEMM_BATCH:
        raise L.DdpError("more (conv, slot) pairs per source array than DDP_MAX_GEMM_BATCH")
    if n_rows == 0:
        return
    args = (x.data_ptr(), x.stride(0), n_rows, ptr(rows), ptr(rows_cnt), out_rows if out_rows is not None else n_rows, st.offs, nb,
            st.W.data_ptr())
    if st.path.rows:
        fn, name = (lib.ddp_stage_a_gh3, "ddp_stage_a_gh3") if st.path.gh_fmt == 1 else (lib.ddp_stage_a_gh, "ddp_stage_a_gh")
        L.check(fn(*args, ptr(st.Wh), n_in, ncols, out.data_ptr(), st.ld, ptr(_RANGE_FLAG), st.gh.data_ptr(), stream()), name)
    elif h2:
        L.check(lib.ddp_stage_a_h2(*args, ptr(st.Wh), n_in, ncols, out.data_ptr(), ncols, ptr(_RANGE_FLAG), stream()), "ddp_stage_a_h2")
    else:
        L.check(lib.ddp_stage_a(*args, ptr(st.W3 if x3 else None), n_in, ncols, out.data_ptr(), ncols, stream()), "ddp_stage_a")


# ------------------------------------------------------------------------------------------------ list primitives
def _hold(j, *objs):
    """The job keeps the tensors whose addresses it carries alive (temporaries handed straight to a job builder would
    otherwise be freed - and their memory handed to the next temporary - before the launch)."""
    j._keep = objs
    return j


def _run_jobs(fn, cls, jobs, what):
    lib = L.load()
    for i in range(0, len(jobs), L.DDP_MAX_LIST_JOBS):
        part = jobs[i:i + L.DDP_MAX_LIST_JOBS]
        arr = (cls * len(part))(*part)
        L.check(getattr(lib, fn)(arr, len(part), stream()), what)


def scan_job(n, flag=None, val=None, rowptr=None, base=0, excl=None, excl2=None, lst=None, total=None, n_dev=None) -> L.ScanJob:
    j = L.ScanJob()
    j.n, j.n_dev, j.flag, j.val, j.rowptr, j.base = n, _p(n_dev), _p(flag), _p(val), _p(rowptr), base
    j.excl, j.excl2, j.list, j.total = _p(excl), _p(excl2), _p(lst), _p(total)
    return _hold(j, flag, val, rowptr, excl, excl2, lst, total, n_dev)


def scan_jobs(jobs: Sequence[L.ScanJob]):
    _run_jobs("ddp_scan_jobs", L.ScanJob, list(jobs), "ddp_scan_jobs")


def mark_job(mask, idx, n, n_dev=None) -> L.MarkJob:
    j = L.MarkJob()
    j.idx, j.n, j.n_dev, j.mask = _p(idx), n, _p(n_dev), _p(mask)
    return _hold(j, idx, n_dev, mask)


def mark_jobs(jobs: Sequence[L.MarkJob]):
    _run_jobs("ddp_mark_jobs", L.MarkJob, list(jobs), "ddp_mark_jobs")


def rowcopy_job(n_rows, keep, old_rowptr, new_rowptr, ins, outs) -> L.RowcopyJob:
    j = L.RowcopyJob()
    j.n_rows, j.keep, j.old_rowptr, j.new_rowptr = n_rows, _p(keep), _p(old_rowptr), _p(new_rowptr)
    for k, (a, b) in enumerate(zip(ins, outs)):
        j.inp[k], j.out[k] = _p(a), _p(b)
    return _hold(j, keep, old_rowptr, new_rowptr, list(ins), list(outs))


def rowcopy_jobs(jobs: Sequence[L.RowcopyJob]):
    _run_jobs("ddp_rowcopy_jobs", L.RowcopyJob, list(jobs), "ddp_rowcopy_jobs")


def select_job(n, mask_a, idx_a, mask_b, idx_b, pays, outs, total, scratch, out_idx=None, n_dev=None, pay_add=None) -> L.SelectJob:
    """scratch: int32 [2 * ((n + 2047) // 2048) + 1]."""
    j = L.SelectJob()
    nb = (n + 2047) // 2048
    j.n, j.n_dev, j.mask_a, j.idx_a, j.mask_b, j.idx_b, j.out_idx = n, _p(n_dev), _p(mask_a), _p(idx_a), _p(mask_b), _p(idx_b), _p(out_idx)
    for k, (a, b) in enumerate(zip(pays, outs)):
        j.pay[k], j.out[k] = _p(a), _p(b)
        j.pay_add[k] = 0 if pay_add is None else pay_add[k]
    j.total = _p(total)
    j.block_count, j.block_off = scratch.data_ptr(), scratch.data_ptr() + 4 * nb
    return _hold(j, n_dev, mask_a, idx_a, mask_b, idx_b, out_idx, list(pays), list(outs), total, scratch)


def select_jobs(jobs: Sequence[L.SelectJob]):
    _run_jobs("ddp_select_jobs", L.SelectJob, list(jobs), "ddp_select_jobs")


def radius_job(x, x_ptr, y, y_batch, r, cap, flags, counts, offsets=None, base=0, total=None, out_query=None, out_x=None,
               capacity=0, graph_div=None, overflow=None) -> L.RadiusJob:
    j = L.RadiusJob()
    j.x, j.x_ptr, j.y, j.y_batch, j.ny = x.data_ptr(), x_ptr.data_ptr(), y.data_ptr(), y_batch.data_ptr(), int(y.shape[0])
    j.r, j.max_neighbors, j.flags, j.graph_div = float(r), int(cap), int(flags), _p(graph_div)
    j.counts, j.offsets, j.base, j.total = _p(counts), _p(offsets), int(base), _p(total)
    j.out_query, j.out_x, j.capacity, j.overflow = _p(out_query), _p(out_x), int(capacity), _p(overflow)
    return _hold(j, x, x_ptr, y, y_batch, graph_div, counts, offsets, total, out_query, out_x, overflow)


def radius_search_jobs(jobs: Sequence[L.RadiusJob]):
    _run_jobs("ddp_radius_search_jobs", L.RadiusJob, list(jobs), "ddp_radius_search_jobs")


def group_job(key, n_items, n_keys, pays, rowptr, perm=None, out_key=None, outs=(), scratch=None, n_dev=None, key_map=None) -> L.GroupJob:
    """scratch: int32 [n_keys + n_items]."""
    j = L.GroupJob()
    j.key, j.n_items, j.n_items_dev, j.n_keys = _p(key), n_items, _p(n_dev), n_keys
    for k, a in enumerate(pays):
        j.pay[k] = _p(a)
    j.rowptr, j.perm, j.out_key, j.key_map, j.scratch = _p(rowptr), _p(perm), _p(out_key), _p(key_map), _p(scratch)
    for k, a in enumerate(outs):
        j.out[k] = _p(a)
    return _hold(j, key, n_dev, list(pays), rowptr, perm, out_key, list(outs), key_map, scratch)


def group_jobs(jobs: Sequence[L.GroupJob]):
    _run_jobs("ddp_group_by_key_jobs", L.GroupJob, list(jobs), "ddp_group_by_key_jobs")


def front_lists(*, n_graphs, sizes, maxes, pos, ptrs, r_lig, r_cross, cross_div, neighbors, e_bond, ll, lr, la, tor, touched, near_rows,
                cnt_near, rp_lr, rp_la, views, scratch, flags=0) -> bool:
    """ddp_front_lists: the step's pose-dependent edge lists and their views in two launches.  sizes / maxes: (lig, rec, atom, tor)
    node totals and largest per-graph sizes, maxes with the largest per-graph bond-entry count as fifth; pos / ptrs: (lig, rec, atom,
    tor) coordinates and graph pointers (tor None: no torsion graph); ll / lr: (query array, point array, capacity, count) in the
    argument order of the struct, la with the overflow flag as fifth, tor: (q, x, capacity, count, rowptr) or None; views: name ->
    namespace with rp / perm / key / o0 / o1; scratch: int32 [8 * n_graphs].  False: outside the fused form's limits, nothing was
    written and the caller runs the chain of radius_search_jobs / scan_jobs / group_jobs."""
    a = L.FrontLists()
    a.n_graphs = n_graphs
    a.n_lig, a.n_rec, a.n_atom, a.n_tor = sizes
    a.max_lig, a.max_rec, a.max_atom, a.max_tor, a.max_bonds = maxes
    a.lig_pos, a.rec_pos, a.atom_pos, a.tor_pos = (_p(t) for t in pos)
    a.lig_ptr, a.rec_ptr, a.atom_ptr, a.tor_ptr = (_p(t) for t in ptrs)
    a.r_lig, a.r_cross, a.cross_div = float(r_lig), float(r_cross), _p(cross_div)
    a.ll_neighbors, a.tor_neighbors, a.cross_neighbors, a.la_neighbors = neighbors
    a.radius_flags, a.e_bond = int(flags), int(e_bond)
    a.ll0, a.ll1, a.cap_ll, a.cnt_ll = _p(ll[0]), _p(ll[1]), int(ll[2]), _p(ll[3])
    a.lr0, a.lr1, a.cap_lr, a.cnt_lr = _p(lr[0]), _p(lr[1]), int(lr[2]), _p(lr[3])
    a.la0, a.la1, a.cap_la, a.cnt_la, a.overflow = _p(la[0]), _p(la[1]), int(la[2]), _p(la[3]), _p(la[4])
    if tor is not None:
        a.tor_q, a.tor_x, a.cap_tor, a.cnt_tor, a.rp_tor = _p(tor[0]), _p(tor[1]), int(tor[2]), _p(tor[3]), _p(tor[4])
    a.touched, a.near_rows, a.cnt_near, a.rp_lr, a.rp_la = _p(touched), _p(near_rows), _p(cnt_near), _p(rp_lr), _p(rp_la)
    for name, v in views.items():
        f = getattr(a, name)
        f.rowptr, f.perm, f.key, f.out0, f.out1 = _p(v.rp), _p(v.perm), _p(v.key), _p(v.o0), _p(getattr(v, "o1", None))
    a.scratch = _p(scratch)
    taken = C.c_int32(0)
    L.check(L.load().ddp_front_lists(C.byref(a), C.byref(taken), stream()), "ddp_front_lists")
    return bool(taken.value)


def gather_rows(x, idx, n, out, ncols, n_dev=None):
    lib = L.load()
    if n > 0:
        L.check(lib.ddp_gather_rows(x.data_ptr(), x.stride(0), idx.data_ptr(), n, ptr(n_dev), out.data_ptr(), out.stride(0), ncols,
                                    stream()), "ddp_gather_rows")


def flex_mark(a, b, n_edges, e0, n_a_per_graph, n_b_per_graph, mark, pos=None, flag=None, a_too=False, ref_list=False):
    """ddp_flex_mark: mark[a[e]] = 1 where b[e] (a_too: or a[e]) is "off" in its sample - by position (pos) or by an earlier mask (flag)."""
    L.check(L.load().ddp_flex_mark(ptr(pos), ptr(flag), n_b_per_graph, ptr(a), ptr(b), n_edges, e0, n_a_per_graph, int(a_too), int(ref_list),
                                   ptr(mark), stream()), "ddp_flex_mark")


def fallback_rowmap(mark, recv, old_rowptr, new_rowptr, n_edges, n_recv_per_graph, rowmap):
    L.check(L.load().ddp_fallback_rowmap(ptr(mark), ptr(recv), ptr(old_rowptr), ptr(new_rowptr), n_edges, n_recv_per_graph, ptr(rowmap),
                                         stream()), "ddp_fallback_rowmap")


def clean_pair_maps(touched, recv, src, n_edges, e0, n_graphs, n0, rowmap, rows_v, rowptr=None):
    lib = L.load()
    L.check(lib.ddp_clean_pair_maps(touched.data_ptr(), recv.data_ptr(), src.data_ptr(), ptr(rowptr), n_edges, e0, n_graphs, n0,
                                    rowmap.data_ptr(), rows_v.data_ptr(), stream()), "ddp_clean_pair_maps")


# ------------------------------------------------------------------------------------------------ pose evaluation
def _eval_arg(t, dtype, dev, what):
    if t.device != dev or t.dtype != dtype or not t.is_contiguous():
        raise L.DdpError(f"{what}: expected a contiguous {dtype} tensor on {dev}, got {t.dtype} on {t.device}")


def pose_rmsd(pred, ref, perms, sel=None, rmsd=None, best=None):
    """ddp_pose_rmsd: pred [S, rows, 3] fp32, ref [n_ref, 3] fp32, perms int32 atom-major [n, P], sel int32 [n] rows of pred (None:
    rows 0 .. n-1).  Returns (rmsd [S] fp32, best [S] int32), the minimum over the P columns of perms (ties: the lowest column)."""
    dev = pred.device
    S, n, P = pred.shape[0], perms.shape[0], perms.shape[1]
    for t, dt, w in ((pred, torch.float32, "pred"), (ref, torch.float32, "ref"), (perms, torch.int32, "perms")):
        _eval_arg(t, dt, dev, f"pose_rmsd {w}")
    if sel is not None:
        _eval_arg(sel, torch.int32, dev, "pose_rmsd sel")
        if sel.shape != (n,):
            raise L.DdpError("pose_rmsd: sel must have one entry per perms row")
    elif n > pred.shape[1]:
        raise L.DdpError("pose_rmsd: more perms rows than pred rows")
    if pred.dim() != 3 or pred.shape[2] != 3 or ref.dim() != 2 or ref.shape[1] != 3 or perms.dim() != 2:
        raise L.DdpError("pose_rmsd: pred [S, rows, 3], ref [n_ref, 3], perms [n, P]")
    rmsd = torch.empty(S, dtype=torch.float32, device=dev) if rmsd is None else rmsd
    best = torch.empty(S, dtype=torch.int32, device=dev) if best is None else best
    if S == 0:
        return rmsd, best
    L.check(L.load().ddp_pose_rmsd(pred.data_ptr(), S, pred.shape[1] * 3, _p(sel), n, ref.data_ptr(), ref.shape[0], perms.data_ptr(), P,
                                   rmsd.data_ptr(), best.data_ptr(), stream()), "ddp_pose_rmsd")
    return rmsd, best


def pose_contacts(lig, lig_radii, rec, rec_radii, ref_centroid, overlap=0.4, out=None):
    """ddp_pose_contacts: lig [S, n, 3], lig_radii [n], rec [m, 3] (one receptor for all samples) or [S, m, 3] (one per sample),
    rec_radii [m] (< 0: minimum distance only), ref_centroid [3], all fp32.  Returns [S, 4]: clashes, min_cross, min_self, centroid."""
    dev = lig.device
    S, n = lig.shape[0], lig.shape[1]
    for t, w in ((lig, "lig"), (lig_radii, "lig_radii"), (rec, "rec"), (rec_radii, "rec_radii"), (ref_centroid, "ref_centroid")):
        _eval_arg(t, torch.float32, dev, f"pose_contacts {w}")
    if lig.dim() != 3 or lig.shape[2] != 3 or rec.dim() not in (2, 3) or rec.shape[-1] != 3:
        raise L.DdpError("pose_contacts: lig [S, n, 3], rec [m, 3] or [S, m, 3]")
    m = rec.shape[-2]
    if rec.dim() == 3 and rec.shape[0] != S:
        raise L.DdpError("pose_contacts: a per-sample receptor needs one row block per sample")
    if lig_radii.shape != (n,) or rec_radii.shape != (m,) or ref_centroid.numel() != 3:
        raise L.DdpError("pose_contacts: radii / centroid shapes")
    out = torch.empty(S, 4, dtype=torch.float32, device=dev) if out is None else out
    if S == 0:
        return out
    L.check(L.load().ddp_pose_contacts(lig.data_ptr(), S, n, lig_radii.data_ptr(), rec.data_ptr(), m, 3 * m if rec.dim() == 3 else 0,
                                       rec_radii.data_ptr(), float(overlap), ref_centroid.data_ptr(), out.data_ptr(), stream()),
            "ddp_pose_contacts")
    return out


def pairwise_tile(n: int) -> int:
    """Poses per tile of ddp_pose_pairwise_rmsd at n atoms (csrc/ddp_eval.hip, pairwise_tile)."""
    return 8 if n <= 256 else 4 if n <= 512 else 2


def pose_pairwise_rmsd(pos, perms_t, sel=None, out=None):
    """ddp_pose_pairwise_rmsd: pos [S, rows, 3] fp32, perms_t int32 atom-major [n, P], sel int32 [n] rows of pos (None: rows 0 .. n-1).
    Returns dist [S, S] fp32: for i < j what pose_rmsd(pos[j:j+1], pos[i, sel], perms_t, sel) gives, mirrored, zero diagonal."""
    dev = pos.device
    for t, dt, w in ((pos, torch.float32, "pos"), (perms_t, torch.int32, "perms_t")):
        _eval_arg(t, dt, dev, f"pose_pairwise_rmsd {w}")
    if pos.dim() != 3 or pos.shape[2] != 3 or perms_t.dim() != 2:
        raise L.DdpError("pose_pairwise_rmsd: pos [S, rows, 3], perms_t [n, P]")
    S, n, P = pos.shape[0], perms_t.shape[0], perms_t.shape[1]
    if sel is not None:
        _eval_arg(sel, torch.int32, dev, "pose_pairwise_rmsd sel")
        if sel.shape != (n,):
            raise L.DdpError("pose_pairwise_rmsd: sel must have one entry per perms_t row")
    elif n > pos.shape[1]:
        raise L.DdpError("pose_pairwise_rmsd: more perms_t rows than pos rows")
    if out is None:
        out = torch.empty(S, S, dtype=torch.float32, device=dev)
    else:
        _eval_arg(out, torch.float32, dev, "pose_pairwise_rmsd out")
        if out.shape != (S, S):
            raise L.DdpError("pose_pairwise_rmsd: out [S, S]")
    if S == 0:
        return out
    L.check(L.load().ddp_pose_pairwise_rmsd(pos.data_ptr(), S, pos.shape[1] * 3, _p(sel), n, perms_t.data_ptr(), P, out.data_ptr(),
                                            stream()), "ddp_pose_pairwise_rmsd")
    return out


def pose_cluster(dist, order=None, cutoff=2.0):
    """ddp_pose_cluster: dist [S, S] fp32, order int32 [S] pose indices best first (None: 0 .. S-1).  Returns (labels [S], reps [S],
    sizes [S], n_clusters [1]), int32 on dist's device; reps and sizes are -1 past the n_clusters clusters found."""
    dev = dist.device
    _eval_arg(dist, torch.float32, dev, "pose_cluster dist")
    if dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
        raise L.DdpError("pose_cluster: dist [S, S]")
    S = dist.shape[0]
    if order is not None:
        _eval_arg(order, torch.int32, dev, "pose_cluster order")
        if order.shape != (S,):
            raise L.DdpError("pose_cluster: order must have one entry per pose")
    labels, reps, sizes = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    if S == 0:
        return labels, reps, sizes, count
    L.check(L.load().ddp_pose_cluster(dist.data_ptr(), S, _p(order), float(cutoff), labels.data_ptr(), reps.data_ptr(), sizes.data_ptr(),
                                      count.data_ptr(), stream()), "ddp_pose_cluster")
    return labels, reps, sizes, count


# ------------------------------------------------------------------------------------------------ the pose entries: shared argument handling
# Clash relief, the physics score, the interaction profile and the two minimisers all work on S poses of one ligand against a receptor.
# Each wrapper below is a table of (tensor, dtype, shape or None, name of the struct's pointer field) plus its scalars; the three
# functions here do the rest.  Nothing in them downloads a device tensor.
def pose_dims(who, pos, rec, per_sample=False):
    """(dev, S, n, m, rec_stride) of pos [S, n, 3] fp32 and rec [m, 3] (one receptor for all samples: rec_stride 0) or [S, m, 3] (one per
    sample: rec_stride 3 m; per_sample: the only form allowed, as the joint minimiser writes to it)."""
    dev = pos.device
    _eval_arg(pos, torch.float32, dev, f"{who} pos")
    if pos.dim() != 3 or pos.shape[2] != 3:
        raise L.DdpError(f"{who}: pos [S, n, 3]")
    S, n = pos.shape[0], pos.shape[1]
    if rec.dim() not in ((3,) if per_sample else (2, 3)) or rec.shape[-1] != 3 or (rec.dim() == 3 and rec.shape[0] != S):
        raise L.DdpError(f"{who}: rec [S, m, 3], one receptor per sample" if per_sample else f"{who}: rec [m, 3] or [S, m, 3]")
    m = rec.shape[-2]
    return dev, S, n, m, 3 * m if rec.dim() == 3 else 0


def check_tensors(who, dev, want, optional=(), error=L.DdpError):
    """Every row (tensor, dtype, shape or None, name) of `want` is a contiguous tensor of that dtype on `dev` and, where a shape (a tuple)
    is given, of that shape; a row whose tensor is None passes if its name is in `optional` (optional=None: every row may be None) and
    raises otherwise.  The message carries `who` and the row's name."""
    for t, dt, shape, name in want:
        if t is None:
            if optional is None or name in optional:
                continue
            raise error(f"{who} {name}: missing")
        if t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise error(f"{who} {name}: expected a contiguous {dt} tensor on {dev}, got {t.dtype} on {t.device}")
        if shape is not None and tuple(t.shape) != shape:
            raise error(f"{who} {name}: expected {shape}, got {tuple(t.shape)}")


def _pose_args(cls, who, dev, want, optional, config=None, **scalars):
    """The checked argument struct: cls(**scalars), `form` from config (a scoring.ScoreConfig; None: the struct has no form), and the
    address of every row's tensor under the row's name.  The struct holds raw addresses: the caller keeps the tensors alive."""
    check_tensors(who, dev, want, optional)
    a = cls(**scalars)
    if config is not None:
        a.form = L.ScoreForm.from_config(config)
    for t, _, _, name in want:
        setattr(a, name, _p(t) or None)
    return a


# ------------------------------------------------------------------------------------------------ clash relief (csrc/ddp_refine.hip)
def refine_args(pos, anchor, lig_radii, rec, rec_radii, self_pairs=None, overlap=0.4, restraint=0.0, energy=None, grad=None,
                bonds=None, mask_rotate=None, step=None, tr=None, rot=None, tor=None, trial=None, trial_energy=None, trial_grad=None,
                accepted=None, grow=2.0, shrink=0.5, step_max=1024.0) -> L.RefineArgs:
    """ddp_refine_args_t for the three ddp_refine_* entries, shapes and index tables checked here (the kernels trust them): pos, anchor,
    trial [S, n, 3] fp32; lig_radii [n], rec [m, 3] or [S, m, 3], rec_radii [m] fp32; self_pairs uint8 [n, n]; energy, trial_energy
    [S, 4], grad, trial_grad [S, n, 3], step [S] fp64; bonds int32 [T, 2] as refine_bonds returns it (its VALUES are not looked at
    here: that would be a device-to-host copy, i.e. a synchronisation, per call), mask_rotate uint8 [T, n]; tr, rot
    [S, 3], tor [S, T] fp32; accepted int32 [S].  Tensors an entry does not use may be None.  The struct holds raw addresses: the
    caller keeps the tensors alive while it is in use."""
    dev, S, n, m, rec_stride = pose_dims("refine", pos, rec)
    T = 0 if bonds is None else int(bonds.shape[0])
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    want = [(pos, f32, (S, n, 3), "pos"), (anchor, f32, (S, n, 3), "anchor"), (lig_radii, f32, (n,), "lig_radii"), (rec, f32, None, "rec"),
            (rec_radii, f32, (m,), "rec_radii"), (self_pairs, u8, (n, n), "self_pairs"), (energy, f64, (S, 4), "energy"),
            (grad, f64, (S, n, 3), "grad"), (bonds, i32, (T, 2), "bonds"), (mask_rotate, u8, (T, n), "mask_rotate"), (step, f64, (S,), "step"),
            (tr, f32, (S, 3), "tr"), (rot, f32, (S, 3), "rot"), (tor, f32, (S, T), "tor"), (trial, f32, (S, n, 3), "trial"),
            (trial_energy, f64, (S, 4), "trial_energy"), (trial_grad, f64, (S, n, 3), "trial_grad"), (accepted, i32, (S,), "accepted")]
    if T > 0 and mask_rotate is None:
        raise L.DdpError("refine: bonds without mask_rotate")
    return _pose_args(L.RefineArgs, "refine", dev, want, None, n_samples=S, n=n, m=m, rec_stride=rec_stride, n_tor=T, overlap=float(overlap),
                      restraint=float(restraint), grow=float(grow), shrink=float(shrink), step_max=float(step_max))


def refine_bonds(bonds, n: int, device) -> torch.Tensor:
    """The rotatable-bond table of the ddp_refine_* entries: a HOST tensor [T, 2] of atom indices is checked against [0, n) here, on
    the host, and then uploaded as int32 (once per complex).  A table with an entry outside the ligand raises; the device skips such
    an entry without a read, but it is never handed one."""
    b = torch.as_tensor(bonds)
    if b.is_cuda:
        raise L.DdpError("refine bonds: the table is validated on the host - pass the host tensor")
    b = b.reshape(-1, 2).to(torch.int64)
    if b.numel() and (int(b.min()) < 0 or int(b.max()) >= n):
        raise L.DdpError(f"refine bonds: atom index outside [0, {n})")
    return b.to(torch.int32).contiguous().to(device)


def refine_energy(a: L.RefineArgs):
    """ddp_refine_energy: energy (and grad, when given) of a.pos."""
    L.check(L.load().ddp_refine_energy(C.byref(a), stream()), "ddp_refine_energy")


def refine_direction(a: L.RefineArgs):
    """ddp_refine_direction: tr / rot / tor = step * the inertia-scaled descent direction of a.grad at a.pos."""
    L.check(L.load().ddp_refine_direction(C.byref(a), stream()), "ddp_refine_direction")


def refine_accept(a: L.RefineArgs):
    """ddp_refine_accept: the per-sample select between a.pos and a.trial."""
    L.check(L.load().ddp_refine_accept(C.byref(a), stream()), "ddp_refine_accept")


# ------------------------------------------------------------------------------------------------ clash guidance (csrc/ddp_guidance.hip)
def clash_guidance(a: L.GuidanceArgs, st=None):
    """ddp_clash_guidance: the guidance increments of a.pos added to a.upd, on stream `st` (None: the current stream of the current
    device).  guidance.GuidanceWorkspace builds the struct and checks the tensors."""
    L.check(L.load().ddp_clash_guidance(C.byref(a), stream() if st is None else st), "ddp_clash_guidance")


def score_guidance(a: L.ScoreGuidanceArgs, st=None):
    """ddp_score_guidance: the score-guidance increments of a.pos added to a.upd, on stream `st` (None: the current stream of the
    current device).  score_guidance.ScoreGuidanceWorkspace builds the struct and checks the tensors."""
    L.check(L.load().ddp_score_guidance(C.byref(a), stream() if st is None else st), "ddp_score_guidance")


def score_guidance_flex(a: L.ScoreGuidanceFlexArgs, st=None):
    """ddp_score_guidance_flex: the score-guidance increments of a.pos and of the side chains of a.rec added to a.upd and a.upd_sc, on
    stream `st` (None: the current stream of the current device).  score_guidance.ScoreGuidanceFlexWorkspace builds the struct and
    checks the tensors."""
    L.check(L.load().ddp_score_guidance_flex(C.byref(a), stream() if st is None else st), "ddp_score_guidance_flex")


# ------------------------------------------------------------------------------------------------ physics score (csrc/ddp_score.hip)
def pose_score(pos, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, tor_divisor=1.0, self_pairs=None, energy=None, grad=None,
               with_grad=False):
    """ddp_pose_score: pos [S, n, 3], lig_radii [n], rec [m, 3] (one receptor for all samples) or [S, m, 3] (one per sample), rec_radii [m]
    fp32 (negative: untyped); lig_flags [n], rec_flags [m] uint8 (bit 0 hydrophobic, 1 donor, 2 acceptor); self_pairs uint8 [n, n] or
    None; config: scoring.ScoreConfig (the constants of the form).  Returns (energy [S, 7] fp64 = gauss, repulsion, hydrophobic, hbond,
    inter, intra, total; grad [S, n, 3] fp64 or None).  energy / grad: tensors to write into (grad given, or with_grad: the gradient is
    computed)."""
    dev, S, n, m, rec_stride = pose_dims("pose_score", pos, rec)
    if energy is None:
        energy = torch.empty(S, 7, dtype=torch.float64, device=dev)
    if grad is None and with_grad:
        grad = torch.empty(S, n, 3, dtype=torch.float64, device=dev)
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    want = [(pos, f32, (S, n, 3), "pos"), (lig_radii, f32, (n,), "lig_radii"), (lig_flags, u8, (n,), "lig_flags"), (rec, f32, None, "rec"),
            (rec_radii, f32, (m,), "rec_radii"), (rec_flags, u8, (m,), "rec_flags"), (self_pairs, u8, (n, n), "self_pairs"),
            (energy, f64, (S, 7), "energy"), (grad, f64, (S, n, 3), "grad")]
    a = _pose_args(L.ScoreArgs, "pose_score", dev, want, ("self_pairs", "grad"), config, n_samples=S, n=n, m=m, rec_stride=rec_stride,
                   tor_divisor=float(tor_divisor))
    L.check(L.load().ddp_pose_score(C.byref(a), stream()), "ddp_pose_score")
    return energy, grad


# ------------------------------------------------------------------------------------------------ interaction profile (csrc/ddp_profile.hip)
def pose_profile(pos, lig_radii, lig_flags, rec, rec_radii, rec_flags, res_ptr, config, contact_distance=4.5, profile=None, bits=None):
    """ddp_pose_profile: pos, lig_radii, lig_flags, rec ([m, 3] or [S, m, 3]), rec_radii, rec_flags and config as pose_score; res_ptr int32
    [R + 1]: residue r owns the receptor atoms res_ptr[r] .. res_ptr[r + 1] - 1 (its values are not looked at here: the kernel clamps
    them to [0, m]).  Returns (profile [S, R, 7] fp64 = gauss, repulsion, hydrophobic, hbond, energy, d_min, pairs; bits [S, R] uint8:
    bit 0 contact, 1 hydrophobic, 2 hbond).  profile / bits: tensors to write into."""
    dev, S, n, m, rec_stride = pose_dims("pose_profile", pos, rec)
    if res_ptr is None or res_ptr.dim() != 1 or res_ptr.shape[0] < 1:
        raise L.DdpError("pose_profile: res_ptr [R + 1]")
    R = res_ptr.shape[0] - 1
    if profile is None:
        profile = torch.empty(S, R, 7, dtype=torch.float64, device=dev)
    if bits is None:
        bits = torch.empty(S, R, dtype=torch.uint8, device=dev)
    f32, f64, u8 = torch.float32, torch.float64, torch.uint8
    want = [(pos, f32, (S, n, 3), "pos"), (lig_radii, f32, (n,), "lig_radii"), (lig_flags, u8, (n,), "lig_flags"), (rec, f32, None, "rec"),
            (rec_radii, f32, (m,), "rec_radii"), (rec_flags, u8, (m,), "rec_flags"), (res_ptr, torch.int32, (R + 1,), "res_ptr"),
            (profile, f64, (S, R, 7), "profile"), (bits, u8, (S, R), "bits")]
    a = _pose_args(L.ProfileArgs, "pose_profile", dev, want, (), config, n_samples=S, n=n, m=m, rec_stride=rec_stride, n_res=R,
                   contact_distance=float(contact_distance))
    L.check(L.load().ddp_pose_profile(C.byref(a), stream()), "ddp_pose_profile")
    return profile, bits


# ------------------------------------------------------------------------------------------------ fused minimiser (csrc/ddp_minimize.hip)
def _minimize(who, cls, width, pos, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate, step,
              accepted, energy_in, energy_out, iterations, restraint, grow, shrink, step_max, history, grad, side=None):
    """The call of both minimisers: the ligand's table and scalars, energies [S, width].  side (the joint minimiser): a function of
    (S, m) that gives the side chains' rows, those of their names that may be None, and their scalars; with it rec is per sample."""
    dev, S, n, m, rec_stride = pose_dims(who, pos, rec, per_sample=side is not None)
    T = 0 if bonds is None else int(bonds.shape[0])
    iterations = int(iterations)
    if iterations < 0:
        raise L.DdpError(f"{who}: iterations < 0")
    rows, optional, scalars = side(S, m) if side is not None else ([], (), {})
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    want = [(pos, f32, (S, n, 3), "pos"), (anchor, f32, (S, n, 3), "anchor"), (lig_radii, f32, (n,), "lig_radii"), (lig_flags, u8, (n,), "lig_flags"),
            (rec, f32, None, "rec"), (rec_radii, f32, (m,), "rec_radii"), (rec_flags, u8, (m,), "rec_flags"), (self_pairs, u8, (n, n), "self_pairs"),
            (bonds, i32, (T, 2), "bonds"), (mask_rotate, u8, (T, n), "mask_rotate")] + rows + \
           [(step, f64, (S,), "step"), (accepted, i32, (S,), "accepted"), (energy_in, f64, (S, width), "energy_in"),
            (energy_out, f64, (S, width), "energy_out"), (history, f64, (iterations + 1, S), "history"), (grad, f64, (S, n, 3), "grad")]
    optional = ("self_pairs", "history", "grad") + tuple(optional) + (("bonds", "mask_rotate") if T == 0 else ())
    a = _pose_args(cls, who, dev, want, optional, config, n_samples=S, n=n, m=m, rec_stride=rec_stride, n_tor=T, iterations=iterations,
                   restraint=float(restraint), grow=float(grow), shrink=float(shrink), step_max=float(step_max), **scalars)
    L.check(getattr(L.load(), "ddp_" + who)(C.byref(a), stream()), "ddp_" + who)


def pose_minimize(pos, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate, step, accepted,
                  energy_in, energy_out, iterations, restraint=0.0, grow=2.0, shrink=0.5, step_max=1024.0, history=None, grad=None):
    """ddp_pose_minimize: `iterations` iterations of the line search of minimize.py on every pose, in one launch.  pos (in/out), anchor
    [S, n, 3] fp32; lig_radii [n], rec [m, 3] or [S, m, 3], rec_radii [m] fp32; lig_flags [n], rec_flags [m] uint8; self_pairs uint8 [n, n]
    or None; config: scoring.ScoreConfig; bonds int32 [T, 2] as refine_bonds returns it (its values are not looked at here), mask_rotate
    uint8 [T, n]; step [S] fp64 and accepted [S] int32 (in/out); energy_in, energy_out [S, 4], history [iterations + 1, S] or None,
    grad [S, n, 3] or None, fp64.  Shapes and dtypes are checked here; no device tensor is downloaded."""
    _minimize("pose_minimize", L.MinimizeArgs, 4, pos, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds,
              mask_rotate, step, accepted, energy_in, energy_out, iterations, restraint, grow, shrink, step_max, history, grad)


# ------------------------------------------------------------------------------------------------ pose search (csrc/ddp_search.hip)
def _search(who, cls, field, inner, width, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate,
            replicas, cycle0, perturb, u, cur_pos, cur_e, best_pos, best_e, best_cycle, accepted, trace, flags, iterations, temperature,
            step_init, restraint, grow, shrink, step_max, starts, side=None, moving=()):
    """The call of both searches: the descent's struct `inner` under `field` of cls, the chain's tensors, energies [rows, width].  side
    (the flexible search): as for _minimize, with it rec is per sample; moving: its (cur_mov, best_mov, starts_mov)."""
    dev, S, n, m, rec_stride = pose_dims(who, anchor, rec, per_sample=side is not None)
    T = 0 if bonds is None else int(bonds.shape[0])
    replicas, cycle0, iterations = int(replicas), int(cycle0), int(iterations)
    if replicas < 1 or cycle0 < 0 or iterations < 0:
        raise L.DdpError(f"{who}: replicas < 1, cycle0 < 0 or iterations < 0")
    if u is None or u.dim() != 2:
        raise L.DdpError(f"{who}: u [cycles, rows]")
    side_rows, optional, scalars = side(S, m) if side is not None else ([], (), {})
    n_mov, n_sc = scalars.get("n_mov", 0), scalars.get("n_sc", 0)
    Cn, rows = int(u.shape[0]), S * replicas
    f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32
    ligand = [(anchor, f32, (S, n, 3), "anchor"), (lig_radii, f32, (n,), "lig_radii"), (lig_flags, u8, (n,), "lig_flags"), (rec, f32, None, "rec"),
              (rec_radii, f32, (m,), "rec_radii"), (rec_flags, u8, (m,), "rec_flags"), (self_pairs, u8, (n, n), "self_pairs"),
              (bonds, i32, (T, 2), "bonds"), (mask_rotate, u8, (T, n), "mask_rotate")] + side_rows
    chain = [(perturb, f32, (Cn, rows, 6 + T + n_sc), "perturb"), (u, f64, (Cn, rows), "u"), (cur_pos, f32, (rows, n, 3), "cur_pos"),
             (cur_e, f64, (rows, width), "cur_e"), (best_pos, f32, (rows, n, 3), "best_pos"), (best_e, f64, (rows, width), "best_e"),
             (best_cycle, i32, (rows,), "best_cycle"), (accepted, i32, (rows,), "accepted"), (trace, f64, (Cn, rows, 2), "trace"),
             (flags, u8, (Cn, rows), "flags"), (starts, f32, (Cn, rows, n, 3), "starts")]
    if moving:
        chain += [(moving[0], f32, (rows, n_mov, 3), "cur_mov"), (moving[1], f32, (rows, n_mov, 3), "best_mov"),
                  (moving[2], f32, (Cn, rows, n_mov, 3), "starts_mov")]
    a = cls(replicas=replicas, cycles=Cn, cycle0=cycle0, step_init=float(step_init), temperature=float(temperature))
    optional = ("self_pairs",) + tuple(optional) + (("bonds", "mask_rotate") if T == 0 else ())
    setattr(a, field, _pose_args(inner, who, dev, ligand, optional, config, n_samples=S, n=n, m=m, rec_stride=rec_stride, n_tor=T,
                                 iterations=iterations, restraint=float(restraint), grow=float(grow), shrink=float(shrink),
                                 step_max=float(step_max), **scalars))
    check_tensors(who, dev, chain, ("starts", "starts_mov"))
    for t, _, _, name in chain:
        setattr(a, name, _p(t) or None)
    L.check(getattr(L.load(), "ddp_" + who)(C.byref(a), stream()), "ddp_" + who)


def pose_search(anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate, replicas, cycle0, perturb, u,
                cur_pos, cur_e, best_pos, best_e, best_cycle, accepted, trace, flags, iterations, temperature, step_init=1.0, restraint=0.0,
                grow=2.0, shrink=0.5, step_max=1024.0, starts=None):
    """ddp_pose_search: C cycles of the iterated local search of search.py on the replicas * S rows of the S poses `anchor` [S, n, 3]
    fp32, in one launch.  lig_radii ... mask_rotate as pose_minimize; perturb [C, rows, 6 + T] fp32 and u [C, rows] fp64 (C, the cycles
    of this call, is read off their shape); the row state cur_pos, best_pos [rows, n, 3] fp32, cur_e, best_e [rows, 4] fp64, best_cycle,
    accepted int32 [rows] (in/out; cycle0 = 0: written fresh by the kernel); trace [C, rows, 2] fp64, flags uint8 [C, rows]; starts
    [C, rows, n, 3] fp32 or None; iterations: of one descent.  Shapes and dtypes are checked here; no device tensor is downloaded."""
    _search("pose_search", L.SearchArgs, "min", L.MinimizeArgs, 4, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs,
            bonds, mask_rotate, replicas, cycle0, perturb, u, cur_pos, cur_e, best_pos, best_e, best_cycle, accepted, trace, flags, iterations,
            temperature, step_init, restraint, grow, shrink, step_max, starts)


def pose_search_select(best_pos, best_e, best_cycle, replicas, pos_out=None, energy_out=None, replica_out=None, cycle_out=None):
    """ddp_pose_search_select: per pose the replica with the smallest best_e[:, 3] (strict <, in replica order: ties go to the lower
    replica, NaN and +inf are never smaller, none below +inf gives replica 0).  best_pos [S * replicas, n, 3] fp32, best_e [S * replicas,
    4] fp64, best_cycle int32 [S * replicas].  Returns (pos_out [S, n, 3], energy_out [S, 4], replica_out [S], cycle_out [S])."""
    who = "pose_search_select"
    replicas = int(replicas)
    if best_pos.dim() != 3 or best_pos.shape[2] != 3 or replicas < 1 or best_pos.shape[0] % replicas:
        raise L.DdpError(f"{who}: best_pos [S * replicas, n, 3], replicas >= 1")
    dev, rows, n = best_pos.device, best_pos.shape[0], best_pos.shape[1]
    S = rows // replicas
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    pos_out = torch.empty(S, n, 3, dtype=f32, device=dev) if pos_out is None else pos_out
    energy_out = torch.empty(S, 4, dtype=f64, device=dev) if energy_out is None else energy_out
    replica_out = torch.empty(S, dtype=i32, device=dev) if replica_out is None else replica_out
    cycle_out = torch.empty(S, dtype=i32, device=dev) if cycle_out is None else cycle_out
    want = [(best_pos, f32, (rows, n, 3), "best_pos"), (best_e, f64, (rows, 4), "best_e"), (best_cycle, i32, (rows,), "best_cycle"),
            (pos_out, f32, (S, n, 3), "pos_out"), (energy_out, f64, (S, 4), "energy_out"), (replica_out, i32, (S,), "replica_out"),
            (cycle_out, i32, (S,), "cycle_out")]
    a = _pose_args(L.SearchSelectArgs, who, dev, want, (), None, n_samples=S, n=n, replicas=replicas)
    L.check(L.load().ddp_pose_search_select(C.byref(a), stream()), "ddp_pose_search_select")
    return pos_out, energy_out, replica_out, cycle_out


# ------------------------------------------------------------------------------------------------ joint minimiser (csrc/ddp_minimize_flex.hip)
def flex_tables(sc, m: int, device) -> dict:
    """The side-chain tables of ddp_pose_minimize_flex: HOST tensors (a minimize_flex.SidechainTables, or anything with its fields mov,
    edge_idx, sub, mapping, pairs) are checked against the m receptor atoms here, on the host, as refine_bonds checks the ligand's
    bonds, and then uploaded (once per complex).  The device skips an entry outside the receptor without a read, but it is never
    handed one."""
    from .minimize_flex import check_sidechain_tables
    host = {k: torch.as_tensor(getattr(sc, k)) for k in ("mov", "edge_idx", "sub", "mapping", "pairs")}
    if any(t.is_cuda for t in host.values()):
        raise L.DdpError("flex tables: the tables are validated on the host - pass host tensors")
    mov, edge, sub, mapping = (host[k].to(torch.int64) for k in ("mov", "edge_idx", "sub", "mapping"))
    mov, edge, sub, mapping = mov.reshape(-1), edge.reshape(-1, 2), sub.reshape(-1), mapping.reshape(-1, 2)
    try:
        check_sidechain_tables(m, edge, sub, mapping, mov)
    except ValueError as e:
        raise L.DdpError(f"flex tables: {e}") from None
    pairs = host["pairs"]
    if pairs.dtype != torch.uint8 or tuple(pairs.shape) != (mov.shape[0], m):
        raise L.DdpError(f"flex tables: pairs uint8 [{mov.shape[0]}, {m}], got {pairs.dtype} {tuple(pairs.shape)}")
    out = {k: t.to(torch.int32).contiguous().to(device) for k, t in (("mov", mov), ("edge_idx", edge), ("sub", sub), ("mapping", mapping))}
    out["pairs"] = pairs.contiguous().to(device)
    return out


def _flex_side(tables, rec_anchor, restraint_sc, grad_mov=None):
    """The `side` of _minimize and _search for the joint entries: the rows of the side-chain tables (what flex_tables returns; its
    values are not looked at here), rec_anchor and the optional grad_mov, and the side chains' scalars."""
    mov, edge, sub, mapping, pairs = (tables[k] for k in ("mov", "edge_idx", "sub", "mapping", "pairs"))
    n_mov, n_sc, n_sub = int(mov.shape[0]), int(edge.shape[0]), int(sub.shape[0])

    def side(S, m):
        i32 = torch.int32
        rows = [(rec_anchor, torch.float32, (S, m, 3), "rec_anchor"), (mov, i32, (n_mov,), "mov"), (edge, i32, (n_sc, 2), "sc_edge_idx"),
                (sub, i32, (n_sub,), "sc_sub"), (mapping, i32, (n_sc, 2), "sc_map"), (pairs, torch.uint8, (n_mov, m), "sc_pairs"),
                (grad_mov, torch.float64, (S, n_mov, 3), "grad_mov")]
        return rows, ("grad_mov",), dict(n_mov=n_mov, n_sc=n_sc, n_sub=n_sub, restraint_sc=float(restraint_sc))

    return side


def pose_minimize_flex(pos, anchor, lig_radii, lig_flags, rec, rec_anchor, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate,
                       tables, step, accepted, energy_in, energy_out, iterations, restraint=0.0, restraint_sc=0.0, grow=2.0, shrink=0.5,
                       step_max=1024.0, history=None, grad=None, grad_mov=None):
    """ddp_pose_minimize_flex: `iterations` iterations of the joint line search of minimize_flex.py on every pose, in one launch.  As
    pose_minimize, with: rec (in/out) and rec_anchor [S, m, 3] fp32, one receptor per sample; tables: what flex_tables returns (its
    values are not looked at here); energy_in, energy_out [S, 6]; grad_mov [S, n_mov, 3] fp64 or None.  Shapes and dtypes are checked
    here; no device tensor is downloaded."""
    _minimize("pose_minimize_flex", L.MinimizeFlexArgs, 6, pos, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs,
              bonds, mask_rotate, step, accepted, energy_in, energy_out, iterations, restraint, grow, shrink, step_max, history, grad,
              _flex_side(tables, rec_anchor, restraint_sc, grad_mov))


# ------------------------------------------------------------------------------------------------ flexible search (csrc/ddp_search_flex.hip)
def pose_search_flex(anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config, self_pairs, bonds, mask_rotate, tables, replicas, cycle0,
                     perturb, u, cur_pos, cur_mov, cur_e, best_pos, best_mov, best_e, best_cycle, accepted, trace, flags, iterations, temperature,
                     step_init=1.0, restraint=0.0, restraint_sc=0.0, grow=2.0, shrink=0.5, step_max=1024.0, starts=None, starts_mov=None,
                     rec_anchor=None):
    """ddp_pose_search_flex: C cycles of the search of search_flex.py on the replicas * S rows of the S sampled states (anchor [S, n, 3],
    rec [S, m, 3], both fp32 and only read), in one launch.  As pose_search, with: tables: what flex_tables returns; perturb [C, rows,
    6 + T + n_sc]; the moving atoms of the row state cur_mov, best_mov [rows, n_mov, 3] fp32; cur_e, best_e [rows, 6]; starts_mov
    [C, rows, n_mov, 3] or None; rec_anchor [S, m, 3]: the anchor of the side-chain restraint (None: rec, the definition).  Shapes and
    dtypes are checked here; no device tensor is downloaded."""
    _search("pose_search_flex", L.SearchFlexArgs, "flex", L.MinimizeFlexArgs, 6, anchor, lig_radii, lig_flags, rec, rec_radii, rec_flags, config,
            self_pairs, bonds, mask_rotate, replicas, cycle0, perturb, u, cur_pos, cur_e, best_pos, best_e, best_cycle, accepted, trace, flags,
            iterations, temperature, step_init, restraint, grow, shrink, step_max, starts,
            _flex_side(tables, rec if rec_anchor is None else rec_anchor, restraint_sc), (cur_mov, best_mov, starts_mov))


# ------------------------------------------------------------------------------------------------ pocket finder (csrc/ddp_pockets.hip)
def _grid_n(dims) -> int:
    nx, ny, nz = (int(d) for d in dims)
    return nx * ny * nz if min(nx, ny, nz) > 0 else 0


def pocket_occupancy(pos, r2, lo, spacing, dims, occ=None):
    """ddp_pocket_occupancy: pos [N, 3] fp32, r2 [N] fp32 = fp32((radius + probe)^2), lo (3 floats, already fp32 values), dims (nx, ny, nz)
    -> occ uint8 [nx, ny, nz]."""
    dev = pos.device
    _eval_arg(pos, torch.float32, dev, "pocket pos")
    _eval_arg(r2, torch.float32, dev, "pocket r2")
    if pos.dim() != 2 or pos.shape[1] != 3 or r2.shape != pos.shape[:1]:
        raise L.DdpError("pocket_occupancy: pos [N, 3] and r2 [N]")
    nx, ny, nz = (int(d) for d in dims)
    if occ is None:
        occ = torch.empty((max(nx, 0), max(ny, 0), max(nz, 0)), dtype=torch.uint8, device=dev)
    _eval_arg(occ, torch.uint8, dev, "pocket occ")
    if occ.numel() != _grid_n(dims):
        raise L.DdpError("pocket_occupancy: occ does not have the grid's size")
    L.check(L.load().ddp_pocket_occupancy(ptr(pos if pos.numel() else None), ptr(r2 if r2.numel() else None), int(pos.shape[0]), float(lo[0]),
                                          float(lo[1]), float(lo[2]), float(spacing), nx, ny, nz, ptr(occ if occ.numel() else None), stream()),
            "ddp_pocket_occupancy")
    return occ


def pocket_buriedness(occ, spacing, ray_length, min_lines, bur=None, mask=None):
    """ddp_pocket_buriedness: occ uint8 [nx, ny, nz] -> (bur uint8, mask int32: bur + 1 at the pocket points, else 0), same shape."""
    dev = occ.device
    _eval_arg(occ, torch.uint8, dev, "pocket occ")
    if occ.dim() != 3:
        raise L.DdpError("pocket_buriedness: occ [nx, ny, nz]")
    bur = torch.empty_like(occ) if bur is None else bur
    mask = torch.empty(occ.shape, dtype=torch.int32, device=dev) if mask is None else mask
    _eval_arg(bur, torch.uint8, dev, "pocket bur")
    _eval_arg(mask, torch.int32, dev, "pocket mask")
    if bur.shape != occ.shape or mask.shape != occ.shape:
        raise L.DdpError("pocket_buriedness: bur and mask have the grid's shape")
    nx, ny, nz = occ.shape
    some = occ.numel() > 0
    L.check(L.load().ddp_pocket_buriedness(ptr(occ if some else None), nx, ny, nz, float(spacing), float(ray_length), int(min_lines),
                                           ptr(bur if some else None), ptr(mask if some else None), stream()), "ddp_pocket_buriedness")
    return bur, mask


def pocket_label(mask, labels=None):
    """ddp_pocket_label: mask int32 [nx, ny, nz] (non-zero = in the mask) -> labels int32, the smallest flat index of each point's
    6-connected component, -1 outside the mask."""
    dev = mask.device
    _eval_arg(mask, torch.int32, dev, "pocket mask")
    if mask.dim() != 3:
        raise L.DdpError("pocket_label: mask [nx, ny, nz]")
    labels = torch.empty_like(mask) if labels is None else labels
    _eval_arg(labels, torch.int32, dev, "pocket labels")
    if labels.shape != mask.shape:
        raise L.DdpError("pocket_label: labels has the grid's shape")
    nx, ny, nz = mask.shape
    some = mask.numel() > 0
    L.check(L.load().ddp_pocket_label(ptr(mask if some else None), nx, ny, nz, ptr(labels if some else None), stream()), "ddp_pocket_label")
    return labels
