"""diffdock_pocket_amd/search.py without a device, on the torch form (the definition): replica 0 of cycle 0 is the minimiser, bit for
bit; the bookkeeping (flags, running best, selection) replayed in NumPy fp64 from trace and u; the exact inequality against the
minimiser on a hand-made chain and on the 16 perturbed poses of the 3dpf fixture (computed once); resumption and seeds; forced
Metropolis decisions; NaN containment; cycles = 0 and S = 0; the C entries' declaration, export, struct layout and launch-free guards;
the flags and run_csv."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd.sampler import rotate_index_lists
from test_minimize_cpu import bits32, chain_case
from test_refine_cpu import rigid_fragments
from test_scoring_cpu import CFG, CSV, ROOT, _rows, _run, fixture_3dpf, perturbed_poses

_CACHE = {}
STATE_FIELDS = ("cur_pos", "cur_e", "best_pos", "best_e", "best_cycle", "accepted", "trace", "flags", "energy_minimized")
U_HIGH = 1.0 - 2.0 ** -53


# ---------------------------------------------------------------------------------------------- shared helpers and fixtures
def chain_searcher(case, config, device="cpu"):
    """A PoseSearcher on the raw tables of test_minimize_cpu.chain_case (there is no graph behind them): the attributes that
    PoseSearcher.start / advance / select and PoseMinimizer.advance read, and nothing else (no result(): there is no PoseScorer)."""
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = case
    dev = torch.device(device)
    n, T = x.shape[1], bonds.shape[0]
    tab = dict(lig_r=lig_r, lig_f=lig_f, rec=rec, rec_r=rec_r, rec_f=rec_f, pairs=pairs)
    mz = M.PoseMinimizer.__new__(M.PoseMinimizer)
    mz.config = M.MinimizeConfig(iterations=config.iterations, restraint=config.restraint)
    mz.device, mz.score_config, mz.n, mz.n_a, mz.T = dev, CFG, n, rec.shape[0], T
    mz.scorer = types.SimpleNamespace(_cpu=tab, _dev={k: v.to(dev) for k, v in tab.items()} if dev.type != "cpu" else None,
                                      receptor_from_graph=False, _check=lambda lig_pos, atom_pos: None, config=CFG, n=n, n_a=rec.shape[0])
    mz.bonds, mz.mask_rotate = bonds.long(), mask.bool()
    mz.rot_idx = rotate_index_lists(mz.mask_rotate)
    mz._ref_lig = x[0].clone()
    if dev.type != "cpu":
        mz._bonds_i32, mz._mask_u8 = bonds.to(dev), mask.to(dev)
    ps = SE.PoseSearcher.__new__(SE.PoseSearcher)
    ps.config, ps.minimizer, ps.device, ps.scorer, ps.n, ps.T, ps._ref_lig = config, mz, dev, mz.scorer, n, T, mz._ref_lig.to(dev)
    return ps


def replay(trace, u, temperature, R, ec0=None, eb0=None, bc0=None, c0=0):
    """The rules of search.py replayed in NumPy fp64 on trace [C, rows, 2] and u [C, rows]: (flags [C, rows], ec [C + 1, rows] and eb
    [C + 1, rows] before every cycle and after the last, best_cycle [rows], margin = the smallest |u - exp(-(el - ec) / temperature)|
    over the decisions that the random number takes)."""
    C, rows = u.shape
    ec = np.full(rows, np.inf) if ec0 is None else np.array(ec0, dtype=np.float64)
    eb = np.full(rows, np.inf) if eb0 is None else np.array(eb0, dtype=np.float64)
    bc = np.full(rows, -1, dtype=np.int64) if bc0 is None else np.array(bc0, dtype=np.int64)
    flags = np.zeros((C, rows), dtype=np.uint8)
    ecs, ebs, margin = [ec.copy()], [eb.copy()], np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            el = trace[c, :, 1]
            lower = el < ec
            p = np.exp(-(el - ec) / temperature)
            move = lower | (u[c] < p)
            by_u = ~lower & np.isfinite(p)
            if by_u.any():
                margin = min(margin, float(np.abs(u[c] - p)[by_u].min()))
            improved = el < eb
            ec = np.where(move, el, ec)
            eb = np.where(improved, el, eb)
            bc = np.where(improved, c0 + c, bc)
            flags[c] = move.astype(np.uint8) | (improved.astype(np.uint8) << 1)
            ecs.append(ec.copy())
            ebs.append(eb.copy())
    return flags, np.stack(ecs), np.stack(ebs), bc, margin


def select_ref(e3, R):
    """The selection rule, spelled out: strict < in replica order from +inf; none: replica 0."""
    out = []
    for s in range(e3.shape[0] // R):
        best, bv = 0, np.inf
        for r in range(R):
            if e3[s * R + r] < bv:
                best, bv = r, e3[s * R + r]
        out.append(best)
    return np.array(out)


def fixture_search():
    """(PoseSearcher, SearchResult, final state) of the CPU form on the 16-pose fixture, full typed receptor, R = 2, C = 3, K = 10; once."""
    if "run" not in _CACHE:
        g, _, full = fixture_3dpf()
        ps = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig(replicas=2, cycles=3, iterations=10))
        x = perturbed_poses()
        state = ps.advance(ps.start(x), 3)
        _CACHE["run"] = (ps, ps.result(state), state)
    return _CACHE["run"]


def same_state(a, b, what=""):
    for k in STATE_FIELDS:
        ta, tb = getattr(a, k), getattr(b, k)
        if ta.dtype == torch.float64:
            ta, tb = ta.contiguous().view(torch.int64), tb.contiguous().view(torch.int64)
        elif ta.dtype == torch.float32:
            ta, tb = bits32(ta), bits32(tb)
        assert torch.equal(ta, tb), f"{what}: {k}"
    assert a.cycle == b.cycle


# ---------------------------------------------------------------------------------------------- 1. replica 0 is the minimiser
def test_replica_zero_of_cycle_zero_is_the_minimiser_bit_for_bit():
    g, _, full = fixture_3dpf()
    x = perturbed_poses()[:5]
    for K in (0, 6):
        ps = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig(replicas=3, cycles=2, iterations=K))
        st = ps.advance(ps.start(x), 1)
        mz = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=K))
        xm, _, acc, e0, e1 = mz.advance(x, x, torch.ones(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int32), K)
        assert torch.equal(bits32(st.cur_pos[::3]), bits32(xm)) and torch.equal(bits32(st.best_pos[::3]), bits32(xm))
        assert torch.equal(st.cur_e[::3], e1) and torch.equal(st.best_e[::3], e1) and torch.equal(st.energy_minimized, e1)
        assert torch.equal(st.accepted[::3], acc) and torch.equal(st.trace[0, ::3, 0], e0[:, 3]) and torch.equal(st.trace[0, ::3, 1], e1[:, 3])
        assert bool((st.flags[0] == 3).all()) and bool((st.best_cycle == 0).all())
        # the other replicas started somewhere else
        assert not torch.equal(st.trace[0, 1::3, 0], e0[:, 3])


# ---------------------------------------------------------------------------------------------- 2. bookkeeping
def test_flags_best_and_selection_follow_the_rules():
    ps, res, st = fixture_search()
    R, T = 2, ps.config.temperature
    flags, ecs, ebs, bc, margin = replay(st.trace.numpy(), st.u.numpy(), T, R)
    assert margin > 1e-9, margin                       # no decision hangs on the last bits of exp
    assert np.array_equal(flags, st.flags.numpy())
    assert np.array_equal(ebs[-1], st.best_e[:, 3].numpy()) and np.array_equal(ecs[-1], st.cur_e[:, 3].numpy())
    assert np.array_equal(ebs[-1], np.minimum.accumulate(st.trace[:, :, 1].numpy(), 0)[-1])          # the running strict minimum
    assert np.array_equal(bc, st.best_cycle.numpy()) and np.array_equal(bc, np.argmin(st.trace[:, :, 1].numpy(), 0))
    assert 0 < int((st.flags & 1).sum()) < st.flags.numel(), "the fixture has moves and stays"
    rep = select_ref(st.best_e[:, 3].numpy(), R)
    assert np.array_equal(rep, res.replica.numpy()) and len(set(rep.tolist())) == 2, rep
    q = torch.arange(16) * R + res.replica.long()
    assert torch.equal(bits32(res.lig_pos), bits32(st.best_pos[q])) and torch.equal(res.energy_after, st.best_e[q])
    assert torch.equal(res.cycle, st.best_cycle[q]) and torch.equal(res.moves, (st.flags[:, q] & 1).sum(0).to(torch.int32))
    # crafted energies: a tie goes to the lower replica, NaN and +inf are never smaller, all +inf gives replica 0
    inf, nan = float("inf"), float("nan")
    e3 = torch.tensor([1.0, -2.0, -2.0, nan, inf, 5.0, inf, inf, inf, nan, nan, nan])
    be = torch.zeros(12, 4, dtype=torch.float64)
    be[:, 3] = e3
    pos = torch.arange(12 * 2 * 3, dtype=torch.float32).reshape(12, 2, 3)
    p, e, r, c = SE.select_torch(be, pos, torch.arange(12, dtype=torch.int32), 3)
    assert r.tolist() == [1, 2, 0, 0] and c.tolist() == [1, 5, 6, 9] and torch.equal(p, pos[[1, 5, 6, 9]])
    assert r.tolist() == select_ref(e3.numpy(), 3).tolist()


# ---------------------------------------------------------------------------------------------- 3. never worse than the minimiser
def test_the_result_is_never_worse_than_the_minimiser_exactly():
    ps, res, st = fixture_search()
    g, _, full = fixture_3dpf()
    x0 = perturbed_poses()
    mres = M.PoseMinimizer(g, receptor=full, config=M.MinimizeConfig(iterations=10)).minimize(x0)
    assert torch.equal(res.energy_minimized, mres.energy_after) and torch.equal(res.energy_before, mres.energy_before)
    assert bool((res.energy_after[:, 3] <= res.energy_minimized[:, 3]).all()) and bool((res.energy_minimized[:, 3] <= res.energy_before[:, 3]).all())
    assert bool((res.energy_after[:, 3] < res.energy_minimized[:, 3]).any()), "no replica found anything below the plain descent"
    print("E before", [round(float(v), 2) for v in res.energy_before[:, 3]], "\nminimised", [round(float(v), 2) for v in res.energy_minimized[:, 3]],
          "\nsearched", [round(float(v), 2) for v in res.energy_after[:, 3]], "\nreplica", res.replica.tolist(), "cycle", res.cycle.tolist())
    assert torch.equal(res.energy_after[:, 0], res.scores_after.inter) and torch.equal(res.energy_after[:, 1], res.scores_after.intra)
    assert torch.allclose(res.rmsd_moved.double(), (res.lig_pos.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt(), atol=1e-5)
    bonds, _ = R.ligand_torsions(g)
    worst = 0.0
    for frag in rigid_fragments(37, g["ligand", "ligand"].edge_index.numpy(), bonds):
        if len(frag) > 1:
            d0, d1 = torch.cdist(x0[:, frag].double(), x0[:, frag].double()), torch.cdist(res.lig_pos[:, frag].double(), res.lig_pos[:, frag].double())
            worst = max(worst, float((d0 - d1).abs().max()))
    assert worst <= 1e-4, worst
    # the hand-made chain: the same chain of inequalities on the raw state
    for n, T in ((12, 1), (37, 5)):
        case = chain_case(3, n, T, 300, 70 + n)
        cs = chain_searcher(case, SE.SearchConfig(replicas=2, cycles=3, iterations=10, seed=n))
        s = cs.advance(cs.start(case[0]), 3)
        _, e, rep, _ = cs.select(s)
        assert bool((e[:, 3] <= s.energy_minimized[:, 3]).all()) and bool((s.energy_minimized[:, 3] <= s.trace[0, ::2, 0]).all())
        assert bool(torch.isfinite(e[:, 3]).all())


# ---------------------------------------------------------------------------------------------- 4. resumption and seeds
def test_advance_resumes_and_the_seed_decides_the_numbers():
    ps, _, whole = fixture_search()
    x = perturbed_poses()
    fresh = ps.start(x)
    before = {k: getattr(fresh, k).clone() for k in STATE_FIELDS}
    a = ps.advance(fresh, 1)
    same_state(ps.advance(a, 2), whole, "1 + 2")
    same_state(ps.advance(ps.advance(a, 1), 1), whole, "1 + 1 + 1")
    assert all(torch.equal(getattr(fresh, k).nan_to_num(7.0), before[k].nan_to_num(7.0)) for k in STATE_FIELDS) and fresh.cycle == 0
    with pytest.raises(ValueError):
        ps.advance(whole, 1)                           # the state carries the numbers of 3 cycles
    again = ps.start(x)
    assert torch.equal(again.perturb, fresh.perturb) and torch.equal(again.u, fresh.u)
    p, u = SE.draw_random_numbers(ps.config, 32, ps.T)
    assert torch.equal(p, fresh.perturb) and torch.equal(u, fresh.u) and p.shape == (3, 32, 6 + ps.T) and u.dtype == torch.float64
    assert bool((u >= 0).all()) and bool((u < 1).all())
    other, _ = SE.draw_random_numbers(SE.SearchConfig(replicas=2, cycles=3, iterations=10, seed=1), 32, ps.T)
    assert not torch.equal(other, p)
    # the sigmas scale the three blocks
    wide, _ = SE.draw_random_numbers(SE.SearchConfig(replicas=2, cycles=3, sigma_tr=2.0, sigma_rot=0.6, sigma_tor=0.25), 32, ps.T)
    assert torch.equal(wide[..., :6], 2 * p[..., :6]) and torch.equal(wide[..., 6:], 0.5 * p[..., 6:])


# ---------------------------------------------------------------------------------------------- 5. forced decisions
def test_forced_metropolis_decisions():
    ps, _, _ = fixture_search()
    x = perturbed_poses()[:6]
    for value in (0.0, U_HIGH):
        st = ps.start(x)
        st.u.fill_(value)
        out = ps.advance(st, 3)
        move = (out.flags & 1).bool().numpy()
        tr = out.trace.numpy()
        _, ecs, _, _, _ = replay(tr, out.u.numpy(), ps.config.temperature, 2)
        d = tr[:, :, 1] - ecs[:-1]
        if value == 0.0:
            assert np.array_equal(move, np.isfinite(tr[:, :, 1])) and move.all()
        else:
            clear = (d > 1e-6) | (d < 0) | ~np.isfinite(ecs[:-1])
            assert np.array_equal(move[clear], (tr[:, :, 1] < ecs[:-1])[clear]) and (~move).any() and clear.sum() >= 30
            # a chain that only ever moves downhill: ec is the running minimum
            assert np.array_equal(ecs[-1], out.best_e[:, 3].numpy())


# ---------------------------------------------------------------------------------------------- 6. NaN containment
def test_a_nan_sample_keeps_its_pose_and_touches_no_other_sample():
    g, _, full = fixture_3dpf()
    ps = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig(replicas=2, cycles=2, iterations=4))
    x = perturbed_poses()[:4]
    clean = ps.advance(ps.start(x), 2)
    bad = x.clone()
    bad[2, 5, 1] = float("nan")
    got = ps.advance(ps.start(bad), 2)
    for q in (4, 5):
        assert torch.equal(bits32(got.cur_pos[q]), bits32(bad[2])) and torch.equal(bits32(got.best_pos[q]), bits32(bad[2]))
        assert bool((got.best_e[q] == float("inf")).all()) and bool((got.cur_e[q] == float("inf")).all())
        assert int(got.best_cycle[q]) == -1 and int(got.accepted[q]) == 0 and bool((got.flags[:, q] == 0).all())
        assert bool(torch.isnan(got.trace[:, q]).all())
    keep = [0, 1, 2, 3, 6, 7]
    for k in STATE_FIELDS[:6]:
        assert torch.equal(getattr(got, k)[keep], getattr(clean, k)[keep]), k
    assert torch.equal(got.trace[:, keep], clean.trace[:, keep]) and torch.equal(got.flags[:, keep], clean.flags[:, keep])
    res = ps.result(got)
    assert torch.equal(bits32(res.lig_pos[2]), bits32(bad[2])) and int(res.replica[2]) == 0 and int(res.cycle[2]) == -1
    assert float(res.energy_after[2, 3]) == float("inf") and int(res.moves[2]) == 0


# ---------------------------------------------------------------------------------------------- 7. identities
def test_zero_cycles_and_zero_samples_are_the_identity():
    g, _, full = fixture_3dpf()
    x = perturbed_poses()[:3]
    res = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig(replicas=2, cycles=0)).search(x)
    assert torch.equal(bits32(res.lig_pos), bits32(x)) and res.lig_pos.data_ptr() != x.data_ptr()
    assert torch.equal(res.energy_after, res.energy_before) and torch.equal(res.energy_minimized, res.energy_before)
    assert res.replica.tolist() == [0, 0, 0] and res.cycle.tolist() == [-1, -1, -1] and int(res.moves.sum()) == 0
    assert float(res.rmsd_moved.max()) == 0.0 and res.trace.shape == (0, 6, 2) and res.flags.shape == (0, 6)
    assert torch.equal(res.scores_after.total, res.scores_before.total)
    empty = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig(replicas=2, cycles=2, iterations=2)).search(x[:0])
    assert empty.lig_pos.shape == (0, 37, 3) and empty.energy_after.shape == (0, 4) and empty.trace.shape == (2, 0, 2)
    assert empty.replica.shape == (0,) and empty.scores_after.total.shape == (0,)
    for bad in (dict(replicas=0), dict(cycles=-1), dict(iterations=-1), dict(temperature=0.0), dict(temperature=float("inf")),
                dict(temperature=float("nan")), dict(restraint=-1.0), dict(sigma_tr=-1.0)):
        with pytest.raises(ValueError):
            SE.PoseSearcher(g, config=SE.SearchConfig(**bad))
    c = SE.SearchConfig()
    assert (c.replicas, c.cycles, c.iterations, c.temperature, c.sigma_tr, c.sigma_rot, c.sigma_tor, c.seed, c.restraint) == \
        (6, 10, 30, 1.2, 1.0, 0.3, 0.5, 0, 0.0)
    import diffdock_pocket_amd as DP
    assert DP.PoseSearcher is SE.PoseSearcher and DP.SearchConfig is SE.SearchConfig and DP.SearchResult is SE.SearchResult
    # index() reorders the poses and their rows of trace and flags together
    _, full_res, _ = fixture_search()
    order = torch.tensor([3, 0, 15])
    part = full_res.index(order)
    assert torch.equal(part.lig_pos, full_res.lig_pos[order]) and torch.equal(part.trace, full_res.trace[:, [6, 7, 0, 1, 30, 31]])
    assert torch.equal(part.scores_after.total, full_res.scores_after.total[order]) and isinstance(part.cpu(), SE.SearchResult)


# ---------------------------------------------------------------------------------------------- 8. ABI
def _fields_of(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"([a-z_0-9]+)(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entries_are_declared_exported_built_and_guarded():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in ("ddp_pose_search", "ddp_pose_search_select"):
        assert name in declared and name in L.EXPORTS
    assert set(L.EXPORTS) == declared and "#define DDP_ABI_VERSION 17" in header
    assert "ddp_search.hip" in __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _fields_of(header, "ddp_search_args_t") == [f[0] for f in L.SearchArgs._fields_]
    assert _fields_of(header, "ddp_search_select_args_t") == [f[0] for f in L.SearchSelectArgs._fields_]
    # a ddp_minimize_args_t, 4 int32, 2 doubles, 11 pointers; 4 int32, 7 pointers
    assert ctypes.sizeof(L.SearchArgs) == ctypes.sizeof(L.MinimizeArgs) + 16 + 16 + 11 * 8 and ctypes.sizeof(L.SearchSelectArgs) == 16 + 7 * 8
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17
    for name in ("ddp_pose_search", "ddp_pose_search_select"):
        assert hasattr(lib, name)
        getattr(lib, name).argtypes, getattr(lib, name).restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    # the host-side checks need no device: they return before any launch.  Pointers only have to be non-NULL for that.
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def rc(**kw):
        m = L.MinimizeArgs(n_samples=2, n=8, m=5, rec_stride=0, n_tor=1, iterations=2, anchor=p, lig_radii=p, lig_flags=p, rec=p, rec_radii=p,
                           rec_flags=p, self_pairs=p, bonds=p, mask_rotate=p, cutoff=8.0, gauss_offset=0.0, gauss_width=0.8,
                           hydrophobic_good=0.0, hydrophobic_bad=2.5, hbond_good=-0.6, hbond_bad=0.0, w_gauss=-0.045, w_repulsion=0.8,
                           w_hydrophobic=-0.035, w_hbond=-0.6, restraint=0.0, grow=2.0, shrink=0.5, step_max=1024.0)
        a = L.SearchArgs(replicas=3, cycles=0, cycle0=0, step_init=1.0, temperature=1.2, perturb=p, u=p, cur_pos=p, cur_e=p, best_pos=p,
                         best_e=p, best_cycle=p, accepted=p, trace=p, flags=p)
        for k, v in kw.items():
            setattr(m if hasattr(m, k) and not hasattr(a, k) else a, k, v)
        a.min = m
        return lib.ddp_pose_search(ctypes.byref(a), None)

    assert lib.ddp_pose_search(None, None) == -1
    assert rc() == 0 and rc(n_samples=0, replicas=0) == 0                                     # cycles = 0, n_samples = 0: no-ops
    assert rc(n=L.DDP_MINIMIZE_MAX_ATOMS + 1) == -2 and rc(n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1) == -2      # DDP_ELIMIT
    inf, nan = float("inf"), float("nan")
    for bad in (dict(anchor=None), dict(lig_radii=None), dict(lig_flags=None), dict(rec=None), dict(rec_radii=None), dict(rec_flags=None),
                dict(bonds=None), dict(mask_rotate=None), dict(cutoff=0.0), dict(cutoff=nan), dict(n_samples=-1), dict(n=0), dict(m=-1),
                dict(n_tor=-1), dict(rec_stride=14), dict(gauss_width=0.0), dict(hbond_bad=-0.6), dict(iterations=-1), dict(restraint=-0.1),
                dict(restraint=nan), dict(replicas=0), dict(replicas=-2), dict(cycles=-1), dict(cycle0=-1), dict(temperature=0.0),
                dict(temperature=-1.0), dict(temperature=inf), dict(temperature=nan), dict(step_init=0.0), dict(step_init=-1.0),
                dict(step_init=nan), dict(perturb=None), dict(u=None), dict(cur_pos=None), dict(cur_e=None), dict(best_pos=None),
                dict(best_e=None), dict(best_cycle=None), dict(accepted=None), dict(trace=None), dict(flags=None),
                dict(n_samples=1 << 30, replicas=4)):
        for cycles in (0, 3):                          # the checks come before the no-op of cycles = 0 and before any launch
            assert rc(**{"cycles": cycles, **bad}) == -1, bad

    def rc_sel(**kw):
        a = L.SearchSelectArgs(n_samples=2, n=8, replicas=3, best_pos=p, best_e=p, best_cycle=p, pos_out=p, energy_out=p, replica_out=p, cycle_out=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ddp_pose_search_select(ctypes.byref(a), None)

    assert lib.ddp_pose_search_select(None, None) == -1 and rc_sel(n_samples=0) == 0
    for bad in (dict(n_samples=-1), dict(n=0), dict(replicas=0), dict(best_pos=None), dict(best_e=None), dict(best_cycle=None), dict(pos_out=None),
                dict(energy_out=None), dict(replica_out=None), dict(cycle_out=None)):
        assert rc_sel(**bad) == -1, bad
    assert bytes(buf) == bytes(64), "a guard wrote through a pointer"


# ---------------------------------------------------------------------------------------------- 9. flags and driver
SMALL = dict(replicas=2, cycles=2, iterations=3)


def test_flags_parse_and_default_to_off(tmp_path, capsys):
    p = INF._parser()
    a = p.parse_args([])
    assert a.search_poses is False and a.rank_by == "confidence"
    assert (a.search_replicas, a.search_cycles, a.search_iterations, a.search_temperature, a.search_seed) == (6, 10, 30, 1.2, 0)
    a = p.parse_args(["--search_poses", "--search_replicas", "3", "--search_cycles", "4", "--search_iterations", "7", "--search_temperature",
                      "0.5", "--search_seed", "11", "--rank_by", "searched_score"])
    assert a.search_poses is True and (a.search_replicas, a.search_cycles, a.search_iterations, a.search_temperature, a.search_seed) == (3, 4, 7, 0.5, 11)
    assert a.rank_by == "searched_score"
    (tmp_path / "model_parameters.yml").write_text("{}\n")
    for bad in (["--search_replicas", "0"], ["--search_cycles", "-1"], ["--search_iterations", "-1"], ["--search_temperature", "0"]):
        with pytest.raises(SystemExit) as e:
            INF.main(["--protein_path", "p.pdb", "--ligand", "l.sdf", "--model_dir", str(tmp_path)] + bad)
        assert e.value.code == 2 and "--search_replicas must be at least 1" in capsys.readouterr().err
    with pytest.raises(ValueError, match="rank_by"):
        INF.run_csv("none.csv", None, torch.device("cpu"), rank_by="searched")


def test_run_csv_searches_poses_and_leaves_everything_else_alone(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    cfg = SE.SearchConfig(**SMALL)
    plain = _run(str(p), str(tmp_path / "plain"), minimize_poses=M.MinimizeConfig(iterations=3))
    both = _run(str(p), str(tmp_path / "both"), minimize_poses=M.MinimizeConfig(iterations=3), search_poses=cfg)
    g, pdb, full = fixture_3dpf()
    assert len(both) == 2
    for a, b in zip(plain, both):
        assert a.skipped is None and b.skipped is None and a.searched is None and a.searched_pos is None
        assert torch.equal(a.ligand_pos, b.ligand_pos) and torch.equal(a.confidence, b.confidence) and torch.equal(a.order, b.order)
        assert torch.equal(bits32(a.minimized_pos), bits32(b.minimized_pos))
        old = {os.path.basename(f): f for f in a.files}
        new = {os.path.basename(f): f for f in b.files}
        assert set(new) - set(old) == {"searched.csv"} | {f"rank{k}_searched.sdf" for k in range(1, 5)} and set(old) <= set(new)
        assert set(os.listdir(os.path.dirname(b.files[0]))) == set(new) and set(os.listdir(os.path.dirname(a.files[0]))) == set(old)
        for name, path in old.items():
            assert open(path, "rb").read() == open(new[name], "rb").read(), name
        sr = b.searched
        assert isinstance(sr, SE.SearchResult) and not sr.lig_pos.is_cuda and sr.lig_pos.shape == b.ligand_pos.shape
        assert torch.equal(sr.lig_pos, b.searched_pos) and sr.trace.shape == (2, 8, 2) and sr.flags.shape == (2, 8)
        assert bool((sr.energy_after[:, 3] <= sr.energy_minimized[:, 3]).all()) and bool((sr.energy_minimized[:, 3] <= sr.energy_before[:, 3]).all())
        rows = _rows(new["searched.csv"])
        assert O.SEARCHED_COLUMNS == ["rank", "sample", "total_before", "total_after", "energy_before", "energy_minimized", "energy_after",
                                      "best_replica", "best_cycle", "moves", "rmsd_moved"]
        assert list(rows[0].keys()) == O.SEARCHED_COLUMNS and len(rows) == 4
        for r, row in enumerate(rows):
            assert int(row["rank"]) == r + 1 and int(row["sample"]) == int(b.order[r]) and int(row["best_replica"]) == int(sr.replica[r])
            assert int(row["best_cycle"]) == int(sr.cycle[r]) and int(row["moves"]) == int(sr.moves[r])
            for col, val in (("total_before", sr.scores_before.total[r]), ("total_after", sr.scores_after.total[r]),
                             ("energy_before", sr.energy_before[r, 3]), ("energy_minimized", sr.energy_minimized[r, 3]),
                             ("energy_after", sr.energy_after[r, 3])):
                assert abs(float(row[col]) - float(val)) <= 1e-5 * abs(float(val)) + 1e-12, col
            assert abs(float(row["rmsd_moved"]) - float(sr.rmsd_moved[r])) < 1e-4
        from diffdock_pocket_amd import inputs as I
        for r in range(4):
            got = I.ligand_graph(I.parse_sdf(open(new[f"rank{r + 1}_searched.sdf"]).read()))[1] - np.asarray(b.original_center, dtype=np.float64).reshape(1, 3)
            assert np.abs(got - sr.lig_pos[r].double().numpy()).max() < 2e-4
    # the rigid row ran against the full typed PDB, from the sampled poses in sample order, in this package's CPU form
    inv = torch.argsort(both[1].order)
    want = SE.PoseSearcher(g, receptor=full, config=cfg).search(both[1].ligand_pos[inv])
    assert torch.equal(bits32(want.lig_pos), bits32(both[1].searched_pos[inv])) and torch.equal(want.energy_after, both[1].searched.energy_after[inv])
    assert torch.equal(want.scores_before.total, SC.PoseScorer(g, receptor=full).score(both[1].ligand_pos[inv]).total)


def test_rank_by_searched_score_reorders_everything_downstream(tmp_path, monkeypatch):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    cfg = SE.SearchConfig(**SMALL)
    by_conf = _run(str(p), str(tmp_path / "conf"), search_poses=cfg, score_poses=SC.ScoreConfig())
    # rank_by alone implies the search with the default SearchConfig, which is made a small one here to keep the test quick
    monkeypatch.setattr(INF, "SearchConfig", lambda: SE.SearchConfig(**SMALL))
    by_search = _run(str(p), str(tmp_path / "search"), rank_by="searched_score", score_poses=SC.ScoreConfig())
    for a, b in zip(by_conf, by_search):
        assert b.skipped is None and b.searched is not None
        t = b.searched.scores_after.total
        assert bool((t[:-1] <= t[1:]).all()) and sorted(b.order.tolist()) == [0, 1, 2, 3]
        inv_a, inv_b = torch.argsort(a.order), torch.argsort(b.order)
        assert torch.equal(a.ligand_pos[inv_a], b.ligand_pos[inv_b]) and torch.equal(a.scores.total[inv_a], b.scores.total[inv_b])
        assert torch.equal(bits32(a.searched_pos[inv_a]), bits32(b.searched_pos[inv_b]))
        assert b.order.tolist() == SC.rank_order(a.searched.scores_after.total[inv_a]).tolist()
        files = {os.path.basename(f): f for f in b.files}
        assert [int(r["sample"]) for r in _rows(files["searched.csv"])] == b.order.tolist()
        assert [int(r["sample"]) for r in _rows(files["scores.csv"])] == b.order.tolist()
        assert [int(r["sample"]) for r in _rows(files["modes.csv"])] == b.order.tolist()
        assert int(b.clusters.labels[0]) == 0


def test_the_random_numbers_of_a_seed_are_those_of_the_two_earlier_functions():
    """draw_random_numbers(c, rows, T, 0), its flexible alias and the n_sc > 0 block against the bit patterns that
    search.draw_random_numbers and search_flex.draw_random_numbers_flex gave for this seed before they became one function."""
    from diffdock_pocket_amd import search_flex as SF
    c = SE.SearchConfig(cycles=2, seed=1234, sigma_tr=0.75, sigma_rot=0.25, sigma_tor=0.5, sigma_chi=0.125)
    rigid_p = [-1112827513, -1094799157, 1039825712, -1100892598, 1012713075, 1043012234, -1124836471, -1099998236, -1104850829, 1059698811,
               -1089364555, -1111696319, -1112584649, -1095535664, 1042557945, -1090335686, 1058627640, -1114783505, -1090037706, -1093854668,
               1033110668, 1039847514, -1102757193, -1095350298, -1107097606, -1081337046, 1042904919, 1031547265, -1096182928, 1043492177,
               -1096172058, 1058774508, -1081114095, 1059661056, -1084076830, -1100015028, -1106163031, -1114771255, -1081361206, 1044107434,
               1060379116, 1002445074, -1099887749, -1097593117, 1055629625, -1098761416, 1058803731, 1034156101]
    rigid_u = [4589775617074355296, 4582122549441411424, 4602154245079702742, 4599424220006214562, 4606104959535090931, 4602067004820807288]
    flex_p = [-1112827513, -1094799157, 1039825712, -1100892598, 1012713075, 1043012234, -1124836471, -1099998236, -1126405308, 1038240591,
              -1089364555, -1098013391, -1098679639, -1095535664, 1034169337, -1098724294, 1053589579, -1120075457, -1112246882, -1102243276,
              1046349522, 1052515396, -1097600503, -1103738906, -1121012402, -1095053597, 1038218356, 1039935873, -1104571536, 1035103569,
              -1090609959, 1063873762, -1081114095, 1046578859, -1097409044, -1100015028, -1097774423, -1106382647, -1098138422, 1027330218,
              1060379116, 1002445074, -1099887749, -1097593117, -1114103260, -1094394824, -1090310585, -1102999223, 1038941556, 1038924002,
              1040986104, -1117624761, 1062836917, 1046066523, 1049023867, 1035797751, 1023449886, -1104622819, -1100610801, 1038053628]
    flex_u = [4602717274791769084, 4598699351991666856, 4602485700219835424, 4601236618024812176, 4607034778996619500, 4594794340142202592]
    for draw, args, want_p, want_u in ((SE.draw_random_numbers, (c, 3, 2), rigid_p, rigid_u), (SE.draw_random_numbers, (c, 3, 2, 0), rigid_p, rigid_u),
                                       (SF.draw_random_numbers_flex, (c, 3, 2, 0), rigid_p, rigid_u),
                                       (SF.draw_random_numbers_flex, (c, 3, 2, 2), flex_p, flex_u), (SE.draw_random_numbers, (c, 3, 2, 2), flex_p, flex_u)):
        p, u = draw(*args)
        assert p.dtype == torch.float32 and u.dtype == torch.float64 and p.is_contiguous() and u.is_contiguous()
        assert tuple(p.shape) == (2, 3, 8 + (args[3] if len(args) > 3 else 0)) and tuple(u.shape) == (2, 3)
        assert p.view(torch.int32).flatten().tolist() == want_p and u.view(torch.int64).flatten().tolist() == want_u
