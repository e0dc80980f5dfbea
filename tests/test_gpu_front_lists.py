"""ddp_front_lists (csrc/ddp_front_lists.hip) against the chain of list calls it replaces and against the numpy definition of
tests/front_lists_ref.py, bit for bit.  Every output array is a view between guard words of one sentinel-filled allocation; after
the call the words the definition names hold its values and every other word - guards, tails behind a count - holds the sentinel.
Then the forward and the sampler's replayed steps with model.fused_front_lists on and off."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import front_lists_ref as FR
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import launch as K

pytestmark = pytest.mark.gpu

SENT = -0x2152413
GUARD = 8
VIEWS = ("c_ll", "c_la", "c_lr", "so_ll", "so_la", "so_lr")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Arena:
    """The output arrays of one run as views of one sentinel-filled allocation, GUARD words around each."""

    def __init__(self, c, dev):
        self.start, n = {}, 0
        for name, ln in FR.sizes(c).items():
            self.start[name] = (n + GUARD, ln)
            n += GUARD + ln
        host = np.full(n + GUARD, SENT, dtype=np.int32)
        for name, data in (("ll0", c.bond0), ("ll1", c.bond1), ("overflow", np.zeros(1))):      # inputs: the bond prefix, a clear flag
            host[self.start[name][0]:self.start[name][0] + len(data)] = data
        self.init = host
        self.dev = torch.from_numpy(host.copy()).to(dev)

    def __getitem__(self, name):
        if name not in self.start:
            return None
        s, n = self.start[name]
        return self.dev[s:s + n]

    def view(self, name):
        return SimpleNamespace(rp=self[name + ".rp"], perm=self[name + ".perm"], key=self[name + ".key"], o0=self[name + ".o0"],
                               o1=self[name + ".o1"])

    def expected(self, outs):
        exp = self.init.copy()
        for name, o in outs.items():
            s, n = self.start[name]
            assert o.idx.size == 0 or (o.idx.min() >= 0 and o.idx.max() < n), name
            exp[s + o.idx] = o.val
        return exp

    def mismatch(self, exp):
        got = self.dev.cpu().numpy()
        bad = np.nonzero(got != exp)[0]
        lines = []
        for name, (s, n) in self.start.items():
            b = bad[(bad >= s - GUARD) & (bad < s + n + GUARD)]
            if b.size:
                i = int(b[0])
                lines.append(f"{name}[{i - s}] of {n}: got {int(got[i])}, want {int(exp[i])} ({b.size} words)")
        return lines


def _inputs(c, dev):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)       # noqa: E731
    i = SimpleNamespace(lpos=t(c.lpos, torch.float32), rpos=t(c.rpos, torch.float32), apos=t(c.apos, torch.float32),
                        tpos=t(c.tpos, torch.float32) if c.T else None, cut=t(c.cut, torch.float32) if c.cut is not None else None)
    for k, ptr, n in (("l", c.ptr_l, c.nl), ("r", c.ptr_r, c.nr), ("a", c.ptr_a, c.na), ("t", c.ptr_t, c.nt)):
        setattr(i, "ptr_" + k, t(ptr, torch.int32))
        setattr(i, "b32_" + k, t(np.repeat(np.arange(c.B), n), torch.int32))
    return i


def run_fused(c, i, A, dev, flags=0, max_bonds=None):
    tor = (A["tor_q"], A["tor_x"], c.cap_tor, A["cnt.tor"], A["rp_tor"]) if c.T else None
    scratch = torch.empty(8 * c.B, dtype=torch.int32, device=dev)
    taken = K.front_lists(
        n_graphs=c.B, sizes=(c.Nl, c.Nr, c.Na, c.T), maxes=(max(c.nl), max(c.nr), max(c.na), max(c.nt), c.max_bonds if max_bonds is None else max_bonds),
        pos=(i.lpos, i.rpos, i.apos, i.tpos), ptrs=(i.ptr_l, i.ptr_r, i.ptr_a, i.ptr_t if c.T else None), r_lig=c.r_lig, r_cross=c.r_cross,
        cross_div=i.cut, neighbors=(c.ll_nb, c.tor_nb, 10000, 10000), e_bond=c.Eb, ll=(A["ll0"], A["ll1"], c.cap_ll, A["cnt.ll"]),
        lr=(A["lr0"], A["lr1"], c.cap_lr, A["cnt.lr"]), la=(A["la0"], A["la1"], c.cap_la, A["cnt.la"], A["overflow"]), tor=tor,
        touched=A["touched"], near_rows=A["near_rows"], cnt_near=A["cnt.near"], rp_lr=A["rp_lr"], rp_la=A["rp_la"],
        views={k: A.view(k) for k in VIEWS}, scratch=scratch, flags=flags)
    torch.cuda.synchronize()
    return taken


def run_chain(c, i, A, dev, flags=0):
    """The calls engine._front issues for a rigid step: radius_search_jobs, the near-rows scan, both group_jobs calls."""
    e = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)       # noqa: E731
    Nl, Nr, Na = c.Nl, c.Nr, c.Na
    jobs = [K.radius_job(i.lpos, i.ptr_l, i.lpos, i.b32_l, c.r_lig, c.ll_nb, 1 | flags, e(Nl), e(Nl + 1), base=c.Eb, total=A["cnt.ll"],
                         out_query=A["ll1"], out_x=A["ll0"], capacity=c.cap_ll),
            K.radius_job(i.rpos, i.ptr_r, i.lpos, i.b32_l, c.r_cross, 10000, flags, e(Nl), e(Nl + 1), total=A["cnt.lr"], out_query=A["lr0"],
                         out_x=A["lr1"], capacity=c.cap_lr, graph_div=i.cut),
            K.radius_job(i.apos, i.ptr_a, i.lpos, i.b32_l, c.r_lig, 10000, flags, e(Nl), e(Nl + 1), total=A["cnt.la"], out_query=A["la0"],
                         out_x=A["la1"], capacity=c.cap_la, overflow=A["overflow"]),
            K.radius_job(i.lpos, i.ptr_l, i.apos, i.b32_a, c.r_lig, 10000, flags, A["touched"])]
    if c.T:
        jobs.append(K.radius_job(i.lpos, i.ptr_l, i.tpos, i.b32_t, c.r_lig, c.tor_nb, flags, e(c.T), e(c.T + 1), total=A["cnt.tor"],
                                 out_query=A["tor_q"], out_x=A["tor_x"], capacity=c.cap_tor))
    K.radius_search_jobs(jobs)
    K.scan_jobs([K.scan_job(Na, flag=A["touched"], lst=A["near_rows"], total=A["cnt.near"])])
    v = {k: A.view(k) for k in VIEWS}
    g1 = [K.group_job(A["ll0"], c.cap_ll, Nl, [A["ll1"]], v["c_ll"].rp, v["c_ll"].perm, v["c_ll"].key, [v["c_ll"].o0], e(Nl + c.cap_ll), n_dev=A["cnt.ll"]),
          K.group_job(A["lr0"], c.cap_lr, Nl, [], A["rp_lr"], scratch=e(Nl), n_dev=A["cnt.lr"]),
          K.group_job(A["la0"], c.cap_la, Nl, [], A["rp_la"], scratch=e(Nl), n_dev=A["cnt.la"]),
          K.group_job(A["la1"], c.cap_la, Na, [A["la0"]], v["c_la"].rp, v["c_la"].perm, v["c_la"].key, [v["c_la"].o0], e(Na + c.cap_la), n_dev=A["cnt.la"]),
          K.group_job(A["lr1"], c.cap_lr, Nr, [A["lr0"]], v["c_lr"].rp, v["c_lr"].perm, v["c_lr"].key, [v["c_lr"].o0], e(Nr + c.cap_lr), n_dev=A["cnt.lr"])]
    if c.T:
        g1.append(K.group_job(A["tor_q"], c.cap_tor, c.T, [], A["rp_tor"], scratch=e(c.T), n_dev=A["cnt.tor"]))
    K.group_jobs(g1)
    g2 = []
    for name, cap in (("ll", c.cap_ll), ("la", c.cap_la), ("lr", c.cap_lr)):
        cv, so = v["c_" + name], v["so_" + name]
        g2.append(K.group_job(cv.o0, cap, Nl, [cv.key, cv.perm], so.rp, so.perm, so.key, [so.o0, so.o1], e(Nl + cap), n_dev=A["cnt." + name]))
    K.group_jobs(g2)
    torch.cuda.synchronize()


def front(c, i, A, dev, **kw):
    """What the engine does: the fused entry, and the chain when it declines.  Returns whether the fused form ran."""
    taken = run_fused(c, i, A, dev, **kw)
    if not taken:
        assert np.array_equal(A.dev.cpu().numpy(), A.init), "a declined call wrote something"
        run_chain(c, i, A, dev, flags=kw.get("flags", 0))
    return taken


@pytest.mark.parametrize("name", list(FR.CASES))
def test_fused_lists_equal_the_chain_and_the_definition(name):
    dev = _dev()
    c = FR.case(**FR.CASES[name])
    i = _inputs(c, dev)
    Af, Ac = Arena(c, dev), Arena(c, dev)
    assert front(c, i, Af, dev), "the case lies inside the fused form's limits"
    run_chain(c, i, Ac, dev)
    for k in Af.start:
        assert torch.equal(Af[k], Ac[k]), k
    assert torch.equal(Af.dev, Ac.dev)
    exp = Af.expected(FR.front_lists_def(c))
    assert not Af.mismatch(exp), "\n".join(Af.mismatch(exp))
    assert not Ac.mismatch(exp), "\n".join(Ac.mismatch(exp))
    if name == "b2_la_overflow":
        assert int(Af["overflow"][0]) == 1 and int(Af["cnt.la"][0]) > c.cap_la


FALLBACKS = {
    "nearest": (dict(seed=21, nl=[9, 5], nr=[20, 64], na=[70, 65], nt=[2, 1], cut=[9.0, 10.0]), dict(flags=2)),
    "ligand_beyond_lds": (dict(seed=22, nl=[65, 3], nr=[5, 5], na=[64, 10], nt=[1, 1], cut=[9.0, 9.0]), {}),
    "atoms_beyond_lds": (dict(seed=23, nl=[2], nr=[5], na=[L.DDP_FRONT_MAX_ATOM + 1]), {}),
    "receptor_beyond_lds": (dict(seed=24, nl=[2], nr=[L.DDP_FRONT_MAX_REC + 1], na=[64]), {}),
    "bonds_beyond_lds": (dict(seed=25, nl=[6, 4], nr=[5, 5], na=[64, 10], cut=[9.0, 9.0]), dict(max_bonds=L.DDP_FRONT_MAX_BONDS + 1)),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_are_taken_and_give_the_same_arrays(name):
    dev = _dev()
    args, kw = FALLBACKS[name]
    c = FR.case(**args)
    i = _inputs(c, dev)
    Af, Ac = Arena(c, dev), Arena(c, dev)
    assert not front(c, i, Af, dev, **kw), "the entry must decline this call"
    run_chain(c, i, Ac, dev, flags=kw.get("flags", 0))
    assert torch.equal(Af.dev, Ac.dev)
    if name != "nearest":      # (first-in-index-order cases: the definition applies too)
        exp = Af.expected(FR.front_lists_def(c))
        assert not Af.mismatch(exp), "\n".join(Af.mismatch(exp))


def test_flexible_runs_keep_the_chain():
    """The side-chain graph and the per-step atom kNN views of flexible runs are not covered: the engine does not call the entry."""
    from diffdock_pocket_amd.engine import front_lists_fusable
    on, off = SimpleNamespace(fused_front_lists=True), SimpleNamespace(fused_front_lists=False)
    lay = lambda *n: SimpleNamespace(counts_host=n)       # noqa: E731
    size = dict(lay_l=lay(30, 40), lay_r=lay(139, 139), lay_a=lay(1111, 900), max_bonds=80, tor=SimpleNamespace(lay=lay(7, 9)))
    rigid, flex = SimpleNamespace(num_flex=0, sc=None, **size), SimpleNamespace(num_flex=3, sc=SimpleNamespace(), **size)
    assert front_lists_fusable(on, rigid) and not front_lists_fusable(off, rigid) and not front_lists_fusable(on, flex)
    for k, v in (("lay_l", lay(30, 65)), ("lay_r", lay(257,)), ("lay_a", lay(2049,)), ("max_bonds", 257), ("tor", SimpleNamespace(lay=lay(65,)))):
        assert not front_lists_fusable(on, SimpleNamespace(num_flex=0, sc=None, **{**size, k: v})), k


def _sampler_run(cfgname, flex, fused, n_steps):
    import bench
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    dev = _dev()
    sched = get_t_schedule(20)
    g = make_3dpf_complex(seed=0, flexible_sidechains=flex)
    model, kw = bench.build_model(cfgname, flex, dev)
    model.fused_front_lists = fused
    smp = Sampler(model, g, 5, dev, SamplerConfig(inference_steps=20, flexible_sidechains=flex), seed=0)
    smp.randomize()
    res = [[t.clone() for t in smp.scores(float(sched[0]))]]
    stats = [dict(model.last_stats)]
    taken = [bool(stats[0]["front_fused"])]
    for k in range(n_steps):
        smp.step(k, sched)
    if n_steps:
        assert bool(smp._graph)
        res.append([t.clone() for t in smp.scores(float(sched[n_steps]))])
        stats.append(dict(model.last_stats))
        res.append([smp.lig_pos.clone(), smp.atom_pos.clone()])
    smp.close()
    return res, stats, taken


@pytest.mark.parametrize("cfgname,flex,n_steps", [("cfg1", False, 0), ("cfg2", False, 6), ("cfg2", True, 3)])
def test_forward_and_replayed_steps_with_the_switch_on_and_off(cfgname, flex, n_steps):
    """A cfg1 forward; a 5-sample cfg2 batch through two ordinary steps, the capture and three replays; a flexible batch (the switch
    must change nothing there).  Scores, poses and edge counts are equal bit for bit."""
    (a, sa, ta), (b, sb, tb) = _sampler_run(cfgname, flex, True, n_steps), _sampler_run(cfgname, flex, False, n_steps)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    for u, v in zip(sa, sb):
        assert {k: u[k] for k in u if k.startswith("E_")} == {k: v[k] for k in v if k.startswith("E_")}
        assert all(k in u for k in ("E_ll", "E_lr", "E_la"))
    assert ta == [not flex] and tb == [False]
