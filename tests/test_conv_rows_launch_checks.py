"""What ddp_conv_rows refuses, and with which code: the host checks of the row-stationary conv (both operand-image forms) return before
the library makes any HIP call, so the descriptors below carry dummy pointers that are never dereferenced and no GPU is needed."""
import ctypes as C

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import packing as P

EINVAL, ELIMIT = -1, -2          # DDP_EINVAL, DDP_ELIMIT of include/ddp_hip.h
PTR = 0x10000                    # a 16-byte aligned address nobody reads


def _spec(ns, nv, layer=3):
    return P.faster_tp_spec(P.irreps_muls(ns, nv, layer), P.irreps_muls(ns, nv, layer + 1), 3 * ns, factorized=True)


def _task(spec, form, n_edges=100):
    """A task ddp_conv_rows accepts for `spec` (every pointer a dummy)."""
    t = L.ConvTask()
    t.x_src, t.ldx_src, t.n_edges, t.src, t.eid, t.sh, t.msg = PTR, 256, n_edges, PTR, PTR, PTR, PTR
    for sg in range(3):
        t.seg_ptr[sg], t.seg_idx[sg], t.seg_ld[sg], t.seg_n[sg] = PTR, PTR, spec.f_in, spec.f_in // 3
    t.wsh, t.bsp, t.gh[0], t.gh[1] = PTR, PTR, PTR, PTR
    t.gh_fmt, t.rows_form = 0, form
    return t


def _stream_tiles(spec):
    return spec.nct1 + sum(((b.n + 31) // 32) * (b.U if b.nsub > 1 else (b.U + b.ups - 1) // b.ups) for b in spec.blocks if b.ntiles > 0 and b.U > 0)


# name -> (forms it applies to, expected code, edit(shape, tasks, spec) -> replacement (shape, tasks, ntasks) or None).  Each edit puts
# exactly ONE fault into an otherwise acceptable launch of two tasks, so the order of the library's checks cannot matter.
def _null_shape(s, ts, spec):
    return None, ts, len(ts)


def _null_tasks(s, ts, spec):
    return s, None, 2


def _too_many_tasks(s, ts, spec):
    return s, [_task(spec, ts[0].rows_form) for _ in range(L.DDP_MAX_TASKS + 1)], L.DDP_MAX_TASKS + 1


def _other_size_class(s, ts, spec):
    small = _spec(16, 4)
    return small.ctypes_shape(), [_task(small, t.rows_form) for t in ts], len(ts)


def _wrong_nct1(s, ts, spec):
    s.nct1 += 1


def _block_c2(s, ts, spec):
    assert s.blk[0].C == 1 and s.blk[0].out_off + 2 * s.blk[0].n <= s.d_out      # (the block still fits the message row: one fault)
    s.blk[0].C = 2


def _gh_fmt_2(s, ts, spec):
    for t in ts:
        t.gh_fmt = 2


def _mixed_gh_fmt(s, ts, spec):
    ts[1].gh_fmt = 1


def _mixed_form(s, ts, spec):
    ts[1].rows_form = 1 - ts[0].rows_form


def _bias_k_form0(s, ts, spec):
    for t in ts:
        t.rows_bias_k = 1


def _no_wsh(s, ts, spec):
    ts[1].wsh = None


def _sh_unaligned(s, ts, spec):
    ts[0].sh = PTR + 4


def _range_backwards(s, ts, spec):
    assert spec.hid % 16 != 0                                                     # (rows_bias_k itself is acceptable here)
    for t in ts:
        t.rows_bias_k = 1
    ts[1].rows_seg0, ts[1].rows_seg1, ts[1].rows_nts = 2, 1, spec.nct1 + 1


def _nts_too_large(s, ts, spec):
    ts[0].rows_nts = _stream_tiles(spec) + 1


def _range_without_bias_k(s, ts, spec):
    ts[0].rows_seg0, ts[0].rows_seg1, ts[0].rows_nts = 0, 1, spec.nct1 + 1


def _all_empty(s, ts, spec):
    for t in ts:
        t.n_edges = 0


CASES = [("null shape", (0, 1), EINVAL, _null_shape),
         ("null tasks", (0, 1), EINVAL, _null_tasks),
         ("ntasks > DDP_MAX_TASKS", (0, 1), ELIMIT, _too_many_tasks),
         ("shape outside the ns = 60 / 32 classes", (0, 1), EINVAL, _other_size_class),
         ("wrong nct1", (0, 1), EINVAL, _wrong_nct1),
         ("block with C = 2", (0, 1), EINVAL, _block_c2),
         ("gh_fmt = 2", (0, 1), EINVAL, _gh_fmt_2),
         ("tasks with different gh_fmt", (0, 1), EINVAL, _mixed_gh_fmt),
         ("tasks with different rows_form", (0, 1), EINVAL, _mixed_form),
         ("rows_bias_k = 1 with rows_form = 0", (0,), EINVAL, _bias_k_form0),
         ("missing wsh", (0, 1), EINVAL, _no_wsh),
         ("sh not 16-byte aligned", (0, 1), EINVAL, _sh_unaligned),
         ("rows_seg1 <= rows_seg0", (1,), EINVAL, _range_backwards),
         ("rows_nts above the shape's stream tiles", (1,), EINVAL, _nts_too_large),
         ("rows_seg1 > 0 without rows_bias_k", (1,), EINVAL, _range_without_bias_k),
         ("all tasks empty", (0, 1), 0, _all_empty)]


def test_ddp_conv_rows_refuses_malformed_launches_with_their_codes():
    lib = L.load()
    spec = _spec(60, 10)
    assert spec.f_in == spec.hid == 180 and P.rows_supported(spec)
    bad = []
    for name, forms, want, edit in CASES:
        for form in forms:
            shape, tasks = spec.ctypes_shape(), [_task(spec, form), _task(spec, form)]
            ntasks = len(tasks)
            out = edit(shape, tasks, spec)
            if out is not None:
                shape, tasks, ntasks = out
            arr = (L.ConvTask * len(tasks))(*tasks) if tasks is not None else None
            got = lib.ddp_conv_rows(C.byref(shape) if shape is not None else None, arr, ntasks, None)
            if got != want:
                bad.append((name, form, got, want, lib.ddp_last_error().decode(errors="replace")))
    assert not bad, bad
