"""The list-building kernels (csrc/ddp_lists.hip, csrc/ddp_views.hip) at their seams, device-side counts and job tables, against
the numpy definitions of tests/lists_ref.py.  Every comparison is exact.

All device arrays of a test are views into ONE allocation filled with a sentinel: at least 8 guard words in front of and behind
every array, a view optionally 4 bytes off 16-byte alignment.  After the call the positions the definition names must hold its
values and every other word - guards, tails behind a device-side count, inputs - must hold what it held before, bit for bit.

Scan and grouping cases carry the form they take (ddp_scan_jobs' own rule: the small form when every job of the launch has a
capacity of at most 49152, else the general kernel for all of them) in their parameter id; tests/test_lists_ref_cpu.py checks
the tables against that rule."""
import numpy as np
import pytest
import torch

import list_seam_cases as T
import lists_ref as R
from diffdock_pocket_amd import launch as K

pytestmark = pytest.mark.gpu

SENT = -0x2152413          # no definition produces it: outputs are >= 0 except select payloads, which are >= -1007
GUARD = 8


class Seg:
    def __init__(self, arena, name, start, n, data, odd):
        self.arena, self.name, self.start, self.n, self.data, self.odd = arena, name, start, n, data, odd

    @property
    def t(self):
        t = self.arena.dev[self.start:self.start + self.n]
        assert t.data_ptr() % 16 == (4 if self.odd else 0)
        return t

    def f32(self, rows, ld):
        return self.t.view(torch.float32).view(rows, ld)

    def expect(self, out):
        """The definition's positions (and values; None: workspace) of this array."""
        idx = self.start + np.asarray(out.idx, dtype=np.int64)
        assert idx.size == 0 or (idx.min() >= self.start and idx.max() < self.start + self.n), self.name
        if out.val is None:
            self.arena.free[idx] = True
        else:
            val = np.asarray(out.val, dtype=np.int64)
            assert val.size == 0 or (val.min() >= -2 ** 31 and val.max() < 2 ** 31 and not (val == SENT).any()), self.name
            self.arena.exp[idx] = val.astype(np.int32)


class Arena:
    def __init__(self, what):
        self.what, self.segs, self.size = what, [], 0

    def add(self, name, data=None, n=None, odd=False):
        """An input (data: its content) or an output / workspace of n sentinel words."""
        if data is not None:
            data = np.atleast_1d(np.asarray(data, dtype=np.int64))
            n = data.shape[0]
        assert n >= 1
        start = (self.size + 3) // 4 * 4 + GUARD + (1 if odd else 0)
        self.size = start + n + GUARD
        self.segs.append(Seg(self, name, start, n, data, odd))
        return self.segs[-1]

    def upload(self, dev):
        host = np.full(self.size, SENT, dtype=np.int32)
        for s in self.segs:
            if s.data is not None:
                assert s.data.min() >= -2 ** 31 and s.data.max() < 2 ** 31
                host[s.start:s.start + s.n] = s.data.astype(np.int32)
        self.exp, self.free = host.copy(), np.zeros(self.size, dtype=bool)
        self.dev = torch.from_numpy(host).to(dev)
        assert self.dev.data_ptr() % 16 == 0

    def check(self):
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        bad = np.nonzero((got != self.exp) & ~self.free)[0]
        if bad.size:
            starts = np.array([s.start for s in self.segs])
            lines, seen = [], set()
            for i in bad:
                k = int(np.searchsorted(starts - GUARD, i, side="right")) - 1        # the array whose guarded span holds word i
                s = self.segs[max(k, 0)]
                if s.name not in seen:
                    seen.add(s.name)
                    where = "in front" if i < s.start else "behind" if i >= s.start + s.n else f"[{i - s.start}]"
                    lines.append(f"{s.name} {where}: got {int(got[i])}, want {int(self.exp[i])}")
                if len(lines) >= 12:
                    break
            raise AssertionError(f"{self.what}: {bad.size} wrong words in {len(seen)}+ arrays\n  " + "\n  ".join(lines))
        return got


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(seg):
    return None if seg is None else seg.t


# ------------------------------------------------------------------------------------------------ scan
def _run_scan(groups, what):
    ar, rows = Arena(what), []
    for gi, g in enumerate(groups):
        for ji, c in enumerate(g):
            name = f"{what} launch {gi} job {ji}: {c['mode']} n={c['n']} cap={c['cap']} n_dev={c['n_dev']} base={c['base']} odd={c['odd']}"
            m, odd, outs, s = max(c["cap"], 1), c["odd"], T.SCAN_OUTPUTS[c["mode"]], {}
            for k, o in (("flag", "flag"), ("val", "in"), ("rowptr", "in")):
                if k in c:
                    s[k] = ar.add(f"{name} {k}", c[k], odd=odd == o)
            if "excl" in outs:
                s["excl"] = ar.add(f"{name} excl", n=c["cap"] + 1, odd=odd == "excl")
            if "excl2" in outs:
                s["excl2"] = s["val"] if c["mode"] == "val_inplace" else ar.add(f"{name} excl2", n=m, odd=odd == "excl2")
            if "list" in outs:
                s["list"] = ar.add(f"{name} list", n=c["base"] + m)
            s["total"] = ar.add(f"{name} total", n=1)
            if c["n_dev"] is not None:
                s["n_dev"] = ar.add(f"{name} n_dev", c["n_dev"])
            rows.append((c, s))
    ar.upload(_dev())
    jobs = []
    for c, s in rows:
        g = lambda k: _t(s.get(k))      # noqa: E731
        jobs.append(K.scan_job(c["cap"], flag=g("flag"), val=g("val"), rowptr=g("rowptr"), base=c["base"], excl=g("excl"), excl2=g("excl2"),
                               lst=g("list"), total=g("total"), n_dev=g("n_dev")))
        want = R.scan(c["cap"], c["n_dev"], c.get("flag"), c.get("val"), c.get("rowptr"), c["base"])
        for k in T.SCAN_OUTPUTS[c["mode"]]:
            s[k].expect(want[k])
    K.scan_jobs(jobs)                   # one wrapper call: launches of 12 jobs, in order
    ar.check()


@pytest.mark.parametrize("form", ["small", "general"], ids=["small-form", "general-form"])
def test_scan_seams_counts_and_job_tables(form):
    """Six modes x 13 sizes on the segment seams (255 .. 49152), bases 0 / 11, counts equal to, below and above the capacity and
    negative, an empty job between live ones, 80+ jobs in one wrapper call.  general-form: every launch also holds a job of
    capacity 49153, so ddp_scan_jobs_kernel serves all of them (n >= 4097: more than one chunk per wave, the running carry)."""
    _run_scan(T.scan_sweep(form), f"scan {form}-form")


def test_scan_beyond_the_small_form():
    """general-form only: 49153, 53248 (13 full chunks per wave), 53249, 100003 in every mode."""
    _run_scan(T.scan_large(), "scan general-form large")


@pytest.mark.parametrize("form", ["small", "general"], ids=["small-form-scalar", "general-form-scalar"])
def test_scan_odd_views_take_the_scalar_path(form):
    """One of val / rowptr, flag, excl, excl2 on a view 4 bytes off 16-byte alignment, each on its own, in every mode."""
    _run_scan(T.scan_scalar(form), f"scan {form}-form odd-view")


# ------------------------------------------------------------------------------------------------ select
def _select_rows(ar, cases, what):
    rows = []
    for ji, c in enumerate(cases):
        name = f"{what} job {ji}: n={c['cap']} n_dev={c['n_dev']} {c['flags']} {c['form']} pays={len(c['pays'])} drop={c['drop_out']}"
        m, s = max(c["cap"], 1), {}
        for k in ("mask_a", "idx_a", "mask_b", "idx_b"):
            s[k] = None if c[k] is None else ar.add(f"{name} {k}", c[k])
        s["pays"] = [ar.add(f"{name} pay{k}", p) for k, p in enumerate(c["pays"])]
        s["outs"] = [None if k in c["drop_out"] else ar.add(f"{name} out{k}", n=m) for k in range(len(c["pays"]))]
        s["out_idx"] = ar.add(f"{name} out_idx", n=m) if c["out_idx"] else None
        s["total"] = ar.add(f"{name} total", c["total0"])
        s["scratch"] = ar.add(f"{name} scratch", n=2 * ((c["cap"] + 2047) // 2048) + 1)
        s["n_dev"] = None if c["n_dev"] is None else ar.add(f"{name} n_dev", c["n_dev"])
        rows.append((c, s))
    return rows


def _select_jobs(rows):
    jobs = []
    for c, s in rows:
        jobs.append(K.select_job(c["cap"], _t(s["mask_a"]), _t(s["idx_a"]), _t(s["mask_b"]), _t(s["idx_b"]), [p.t for p in s["pays"]],
                                 [_t(o) for o in s["outs"]], s["total"].t, s["scratch"].t, out_idx=_t(s["out_idx"]), n_dev=_t(s["n_dev"]),
                                 pay_add=c["pay_add"]))
        want = R.select(c["cap"], c["n_dev"], c["mask_a"], c["idx_a"], c["mask_b"], c["idx_b"], c["pays"], c["pay_add"])
        for o, w in zip(s["outs"], want["outs"]):
            if o is not None:
                o.expect(w)
        if s["out_idx"] is not None:
            s["out_idx"].expect(want["out_idx"])
        s["total"].expect(want["total"])
        s["scratch"].expect(R.Out(np.arange(s["scratch"].n), None))
    return jobs


def test_select_seams_and_forms():
    """12 sizes on the ballot-round / wave / block seams x 5 flag patterns, the four mask forms, 0 - 4 payloads with absent
    outputs, out_idx absent, pay_add, counts of 2048 under a capacity of 6145, 0 and above the capacity."""
    ar = Arena("select sweep")
    rows = _select_rows(ar, T.select_sweep(), "select sweep")
    ar.upload(_dev())
    K.select_jobs(_select_jobs(rows))
    ar.check()


def test_select_job_tables():
    """12 live jobs of different sizes in one launch; 13 jobs (split); n == 0 jobs first, in the middle and last with totals of
    their own - the scan's and the scatter's job tables both skip them."""
    ar = Arena("select tables")
    calls = [_select_rows(ar, cases, f"select call {ci}") for ci, cases in enumerate(T.select_tables())]
    ar.upload(_dev())
    for rows in calls:
        K.select_jobs(_select_jobs(rows))
    ar.check()


# ------------------------------------------------------------------------------------------------ mark, rowcopy, gather_rows
def test_mark_jobs():
    """idx absent, repeated indices, n on 255 / 256 / 257, device-side counts, three jobs per launch around an empty one, two jobs
    into one mask; untouched entries keep their prefill of 5."""
    ar = Arena("mark")
    masks, calls = {}, []
    for ci, call in enumerate(T.mark_calls()):
        rows = []
        for ji, j in enumerate(call):
            name = f"mark launch {ci} job {ji}: n={j['n']} n_dev={j['n_dev']} idx={'yes' if j['idx'] is not None else 'none'}"
            if j["mask"] not in masks:
                masks[j["mask"]] = ar.add(f"{name} mask {j['mask']}", np.full(T.MARK_MASK, 5))
            rows.append((j, None if j["idx"] is None else ar.add(f"{name} idx", j["idx"]),
                         None if j["n_dev"] is None else ar.add(f"{name} n_dev", j["n_dev"])))
        calls.append(rows)
    ar.upload(_dev())
    for rows in calls:
        K.mark_jobs([K.mark_job(masks[j["mask"]].t, _t(ix), j["n"], _t(nd)) for j, ix, nd in rows])
        for j, _, _ in rows:
            masks[j["mask"]].expect(R.mark(j["n"], j["n_dev"], j["idx"])["mask"])
    ar.check()


def test_rowcopy_jobs():
    """n_rows 1 .. 129 (4 rows per block), row lengths around the 64-lane stride, keep all / none / random / first and last, 1 - 3
    arrays, a dozen jobs per launch with a zero-row job between them."""
    ar = Arena("rowcopy")
    calls = []
    for ci, call in enumerate(T.rowcopy_calls()):
        rows = []
        for ji, j in enumerate(call):
            name = f"rowcopy launch {ci} job {ji}: n_rows={j['n_rows']} arrays={len(j['ins'])}"
            new = R.scan(j["n_rows"], flag=j["keep"], rowptr=j["old_rowptr"])["excl"].val
            s = dict(keep=ar.add(f"{name} keep", j["keep"]), old=ar.add(f"{name} old_rowptr", j["old_rowptr"]), new=ar.add(f"{name} new_rowptr", new),
                     ins=[ar.add(f"{name} in{k}", x) for k, x in enumerate(j["ins"])],
                     outs=[ar.add(f"{name} out{k}", n=max(j["n_edges"], 1)) for k in range(len(j["ins"]))])
            rows.append((j, new, s))
        calls.append(rows)
    ar.upload(_dev())
    for rows in calls:
        K.rowcopy_jobs([K.rowcopy_job(j["n_rows"], s["keep"].t, s["old"].t, s["new"].t, [x.t for x in s["ins"]], [x.t for x in s["outs"]])
                        for j, _, s in rows])
        for j, new, s in rows:
            for o, w in zip(s["outs"], R.rowcopy(j["n_rows"], j["keep"], j["old_rowptr"], new, j["ins"])["outs"]):
                o.expect(w)
    ar.check()


def test_gather_rows_bits():
    """ncols around the 64-lane stride with padded leading dimensions, n around the 4 rows of a block, repeated indices, counts
    below n / 0 / above; NaN payloads and -0.0 arrive bit for bit, padding columns and rows behind the count stay untouched."""
    ar = Arena("gather_rows")
    rows = []
    for c in T.gather_cases():
        name = f"gather_rows ncols={c['ncols']} n={c['n']} n_dev={c['n_dev']}"
        rows.append((c, ar.add(f"{name} x", c["x"].reshape(-1)), ar.add(f"{name} idx", c["idx"]), ar.add(f"{name} out", n=c["n"] * c["ldo"]),
                     None if c["n_dev"] is None else ar.add(f"{name} n_dev", c["n_dev"])))
    ar.upload(_dev())
    for c, x, idx, out, nd in rows:
        K.gather_rows(x.f32(c["rows"], c["ldx"]), idx.t, c["n"], out.f32(c["n"], c["ldo"]), c["ncols"], n_dev=_t(nd))
        out.expect(R.gather_rows(c["x"], c["idx"], c["n"], c["n_dev"], c["ncols"], c["ldo"])["out"])
    ar.check()


# ------------------------------------------------------------------------------------------------ sharing maps
def test_clean_pair_maps_both_forms():
    """Without rowptr and with it (rowptr cases: touched receivers with row lengths other than sample 0's), E < n0 (the grid is
    sized by n0), E = 256 / 257, B = 1, an atom touched in every sample."""
    ar = Arena("clean_pair_maps")
    rows = []
    for c in T.clean_cases():
        name = f"clean_pair_maps {'rowptr' if c['rowptr'] is not None else 'no-rowptr'} B={c['B']} n0={c['n0']} e0={c['e0']}"
        rows.append((c, {k: ar.add(f"{name} {k}", c[k]) for k in ("touched", "recv", "src", "rowptr") if c[k] is not None},
                     ar.add(f"{name} rowmap", n=c["E"]), ar.add(f"{name} rows_v", n=c["n0"])))
    ar.upload(_dev())
    for c, s, rowmap, rows_v in rows:
        K.clean_pair_maps(s["touched"].t, s["recv"].t, s["src"].t, c["E"], c["e0"], c["B"], c["n0"], rowmap.t, rows_v.t, rowptr=_t(s.get("rowptr")))
        want = R.clean_pair_maps(c["touched"], c["recv"], c["src"], c["E"], c["e0"], c["B"], c["n0"], c["rowptr"])
        rowmap.expect(want["rowmap"])
        rows_v.expect(want["rows_v"])
    ar.check()


def test_flex_mark_shapes_and_bitwise_positions():
    """n_a = 23 against n_b = 57 (receptor<-atom), n_edges < n_a_per_graph, edge counts across 256; by position - displaced, one
    coordinate one ulp away, -0.0 against +0.0 (a difference: the comparison is of bit patterns) - and by flag."""
    ar = Arena("flex_mark")
    rows = []
    for c in T.flex_cases():
        name = f"flex_mark {c['how']} B={c['B']} n_a={c['n_a']} n_b={c['n_b']} e0={c['e0']} a_too={c['a_too']} ref_list={c['ref_list']}"
        rows.append((c, ar.add(f"{name} a", c["a"]), ar.add(f"{name} b", c["b"]),
                     None if c["pos"] is None else ar.add(f"{name} pos", c["pos"].reshape(-1)),
                     None if c["flag"] is None else ar.add(f"{name} flag", c["flag"]), ar.add(f"{name} mark", n=c["B"] * c["n_a"])))
    ar.upload(_dev())
    for c, a, b, pos, flag, mark in rows:
        K.flex_mark(a.t, b.t, c["n_edges"], c["e0"], c["n_a"], c["n_b"], mark.t, pos=None if pos is None else pos.f32(c["B"] * c["n_b"], 3),
                    flag=_t(flag), a_too=c["a_too"], ref_list=c["ref_list"])
        mark.expect(R.flex_mark(c["a"], c["b"], c["n_edges"], c["e0"], c["n_a"], c["n_b"], pos=c["pos"], flag=c["flag"], a_too=c["a_too"],
                                ref_list=c["ref_list"])["mark"])
    ar.check()


def test_fallback_rowmap_edge_counts():
    """1, 255 and 257 edges; unmarked receivers read their sample-0 copy's rows."""
    ar = Arena("fallback_rowmap")
    rows = []
    for c in T.fallback_cases():
        name = f"fallback_rowmap B={c['B']} n={c['n']} edges={c['n_edges']}"
        rows.append((c, {k: ar.add(f"{name} {k}", c[k]) for k in ("mark", "recv", "old_rowptr", "new_rowptr")}, ar.add(f"{name} rowmap", n=c["n_edges"])))
    ar.upload(_dev())
    for c, s, rowmap in rows:
        K.fallback_rowmap(s["mark"].t, s["recv"].t, s["old_rowptr"].t, s["new_rowptr"].t, c["n_edges"], c["n"], rowmap.t)
        rowmap.expect(R.fallback_rowmap(c["mark"], c["recv"], c["old_rowptr"], c["new_rowptr"], c["n_edges"], c["n"])["rowmap"])
    ar.check()


# ------------------------------------------------------------------------------------------------ group_by_key
def _run_group(jobs, what):
    ar, rows = Arena(what), []
    for ji, c in enumerate(jobs):
        name = (f"{what} job {ji}: n_items={c['n_items']} n_dev={c['n_dev']} n_keys={c['n_keys']} perm={c['perm']} "
                f"odd_rowptr={c['odd_rowptr']}")
        m = max(c["n_items"], 1)
        s = dict(key=ar.add(f"{name} key", c["key"]), pays=[ar.add(f"{name} pay{k}", p) for k, p in enumerate(c["pays"])],
                 key_map=None if c["key_map"] is None else ar.add(f"{name} key_map", c["key_map"]),
                 rowptr=ar.add(f"{name} rowptr", n=c["n_keys"] + 1, odd=c["odd_rowptr"]),
                 perm=ar.add(f"{name} perm", n=m) if c["perm"] else None, out_key=ar.add(f"{name} out_key", n=m) if c["out_key"] else None,
                 outs=[ar.add(f"{name} out{k}", n=m) if c["perm"] and k not in c["drop_out"] else None for k in range(len(c["pays"]))],
                 scratch=ar.add(f"{name} scratch", n=c["n_keys"] + (c["n_items"] if c["perm"] else 0)),
                 n_dev=None if c["n_dev"] is None else ar.add(f"{name} n_dev", c["n_dev"]))
        rows.append((c, s))
    ar.upload(_dev())
    gj = []
    for c, s in rows:
        gj.append(K.group_job(s["key"].t, c["n_items"], c["n_keys"], [p.t for p in s["pays"]], s["rowptr"].t, _t(s["perm"]), _t(s["out_key"]),
                              [_t(o) for o in s["outs"]], s["scratch"].t, n_dev=_t(s["n_dev"]), key_map=_t(s["key_map"])))
        want = R.group_by_key(c["key"], c["n_items"], c["n_dev"], c["n_keys"], c["pays"], c["key_map"], perm=c["perm"])
        s["rowptr"].expect(want["rowptr"])
        s["scratch"].expect(want["scratch"])
        if c["perm"]:
            s["perm"].expect(want["perm"])
            if s["out_key"] is not None:
                s["out_key"].expect(want["out_key"])
            for o, w in zip(s["outs"], want["outs"]):
                if o is not None:
                    o.expect(w)
    K.group_jobs(gj)
    return ar.check(), ar.free


@pytest.mark.parametrize("form,jobs", T.group_calls(), ids=["small-form", "general-form"])
def test_group_by_key_jobs_seams(form, jobs):
    """12 jobs per launch - with perm and rowptr-only, an empty one in the middle, rowptr on odd views, key_map, payload subsets,
    rows of 65 / 130 / 200 / 3000 items, counts of 255 / 256 / 257 / 0.  general-form: the launch holds n_keys of 49153 and
    60000, so the in-place scan of the row counters (val == excl2 == scratch) runs in ddp_scan_jobs_kernel for every job.
    Run twice: the slot atomics land in any order, the results may not depend on it."""
    assert T.group_form(jobs) == form
    got1, free = _run_group(jobs, f"group_by_key {form}-form")
    got2, _ = _run_group(jobs, f"group_by_key {form}-form, second run")
    assert np.array_equal(got1[~free], got2[~free])
