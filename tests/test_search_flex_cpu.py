"""diffdock_pocket_amd/search_flex.py without a device, on the torch form (the definition): without side chains it is PoseSearcher bit
for bit; replica 0 of cycle 0 is FlexPoseMinimizer bit for bit; the decisions replayed in NumPy fp64 from trace and u; the exact
inequality on the flexible 3dpf fixture; resumption, seeds and the scales of the random numbers; NaN containment; the static receptor
atoms; the C entry's declaration, export, struct layout and launch-free guards; the flags and run_csv."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flexmin_ref as F
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd import search_flex as SF
from diffdock_pocket_amd.batch import Store
from diffdock_pocket_amd.sampler import apply_sidechain_torsions
from diffdock_pocket_amd.synthetic import make_3dpf_complex
from test_evaluation_cpu import graph_3dpf
from test_minimize_cpu import bits32, chain_case
from test_minimize_flex_cpu import small_flexible_case
from test_scoring_cpu import CFG, CSV, ROOT, _rows, _run, perturbed_poses
from test_search_cpu import _fields_of, chain_searcher, replay, select_ref

_CACHE = {}
STATE_FIELDS = ("cur_pos", "cur_mov", "cur_e", "best_pos", "best_mov", "best_e", "best_cycle", "accepted", "trace", "flags", "energy_minimized")


# ---------------------------------------------------------------------------------------------- shared helpers and fixtures
def chain_torsions(n, T):
    """A ligand torsion table of the kind test_minimize_cpu.chain_case builds: bond j = (2 j + 2, 2 j + 1) turns the atoms behind it."""
    assert 2 * T < n or T == 0
    bonds = torch.tensor([[2 * j + 2, 2 * j + 1] for j in range(T)], dtype=torch.int32).reshape(T, 2)
    mask = torch.zeros(T, n, dtype=torch.uint8)
    for j in range(T):
        mask[j, 2 * j + 2:] = 1
    return bonds, mask


def empty_tables(m):
    return MF.SidechainTables(torch.zeros(0, dtype=torch.long), torch.zeros(0, 2, dtype=torch.long), torch.zeros(0, dtype=torch.long),
                              torch.zeros(0, 2, dtype=torch.long), torch.zeros(0, m, dtype=torch.uint8))


def case_tables(c):
    """The SidechainTables of a flexmin_ref.random_case."""
    return MF.SidechainTables(torch.from_numpy(c["mov"]), torch.from_numpy(c["edge"]), torch.from_numpy(c["sub"]), torch.from_numpy(c["mapping"]),
                              torch.from_numpy(c["sc_pairs"]))


def flex_chain_searcher(case, tables, config, device="cpu"):
    """A FlexPoseSearcher on raw tables (there is no graph behind them): `case` as test_minimize_cpu.chain_case returns it, with rec
    [m, 3] the reference receptor, and a SidechainTables; the attributes that start / advance / select read, and nothing else (no
    result(): there is no PoseScorer)."""
    ps = chain_searcher(case, config, device)
    rigid = ps.minimizer
    fm = MF.FlexPoseMinimizer.__new__(MF.FlexPoseMinimizer)
    fm.rigid = rigid
    fm.config = M.MinimizeConfig(iterations=config.iterations, restraint=config.restraint, sidechain_restraint=config.sidechain_restraint)
    fm.device, fm.scorer, fm.score_config, fm.n, fm.n_a, fm.sc = rigid.device, rigid.scorer, CFG, rigid.n, rigid.n_a, tables
    fm._ref_rec = case[3].float().reshape(-1, 3)
    if torch.device(device).type != "cpu":
        from diffdock_pocket_amd import launch as LA
        fm._sc_dev = LA.flex_tables(tables, rigid.n_a, torch.device(device))
    fs = SF.FlexPoseSearcher.__new__(SF.FlexPoseSearcher)
    fs.config, fs.minimizer = config, fm
    fs._bind()
    return fs


def random_flex_searcher(c, T, config, device="cpu"):
    """flex_chain_searcher on a flexmin_ref.random_case with a chain torsion table: (searcher, x [S, n, 3], y [S, m, 3])."""
    bonds, mask = chain_torsions(c["x"].shape[1], T)
    t = {k: torch.from_numpy(c[k]) for k in ("x", "y", "lig_r", "lig_f", "rec_r", "rec_f")}
    pairs = None if c["pairs"] is None else torch.from_numpy(c["pairs"])
    case = (t["x"], t["lig_r"], t["lig_f"], t["y"][0].contiguous(), t["rec_r"], t["rec_f"], pairs, bonds, mask)
    return flex_chain_searcher(case, case_tables(c), config, device), t["x"], t["y"]


def flex_fixture():
    """(graph, 16 poses, atom_pos [16, m, 3]) on the real 3dpf complex with the flexible residues A:160, A:193 and A:197 (7 moving atoms,
    4 side-chain bonds), the side chains of every pose perturbed by chi noise N(0, 0.3 rad) of torch.Generator().manual_seed(4): the
    inputs of test_gpu_minimize_flex.flex_fixture, built once."""
    if "fix" not in _CACHE:
        g, _ = graph_3dpf("A:160-A:193-A:197")
        fr = g["flexResidues"]
        chi = 0.3 * torch.randn(16, fr.edge_idx.shape[0], generator=torch.Generator().manual_seed(4))
        apos = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(16, 1, 1), fr.edge_idx, fr.subcomponents, fr.subcomponentsMapping, chi)
        _CACHE["fix"] = (g, perturbed_poses(), apos.contiguous())
    return _CACHE["fix"]


FIX = dict(sidechains=True, replicas=2, cycles=3, iterations=6)


def fixture_search():
    """(FlexPoseSearcher, FlexSearchResult, final state) of the CPU form on 6 poses of the flexible fixture, R = 2, C = 3, K = 6; once."""
    if "run" not in _CACHE:
        g, x, y = flex_fixture()
        fs = SF.FlexPoseSearcher(g, config=SE.SearchConfig(**FIX))
        state = fs.advance(fs.start(x[:6], y[:6]), 3)
        _CACHE["run"] = (fs, fs.result(state), state)
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


# ---------------------------------------------------------------------------------------------- 1. the two parents
def test_without_side_chains_it_is_pose_searcher_bit_for_bit():
    """Empty tables, on a graph (n_mov = n_sc = 0 from an empty flexResidues) and on synthetic tables: poses, E, trace, flags."""
    _, lig, apos = small_flexible_case()
    g0 = make_3dpf_complex(seed=2, flexible_sidechains=True, n_lig=12, n_rec=8)
    g0["flexResidues"] = Store(edge_idx=torch.zeros(0, 2, dtype=torch.long), subcomponents=torch.zeros(0, dtype=torch.long),
                               subcomponentsMapping=torch.zeros(0, 2, dtype=torch.long))
    cfg = SE.SearchConfig(sidechains=True, replicas=2, cycles=3, iterations=4, restraint=0.2, sidechain_restraint=0.5, seed=5)
    fs = SF.FlexPoseSearcher(g0, config=cfg)
    assert fs.n_mov == 0 and fs.n_sc == 0
    a = fs.search(lig, apos)
    b = SE.PoseSearcher(g0, receptor="graph", config=cfg).search(lig, apos)
    assert isinstance(a, SF.FlexSearchResult) and torch.equal(bits32(a.lig_pos), bits32(b.lig_pos)) and torch.equal(bits32(a.atom_pos), bits32(apos))
    for k in ("energy_before", "energy_minimized", "energy_after"):
        assert torch.equal(getattr(a, k)[:, [0, 1, 3, 5]], getattr(b, k)) and torch.equal(getattr(a, k)[:, [2, 4]], torch.zeros(3, 2, dtype=torch.float64)), k
    assert torch.equal(a.trace, b.trace) and torch.equal(a.flags, b.flags) and torch.equal(a.replica, b.replica) and torch.equal(a.cycle, b.cycle)
    assert torch.equal(a.moves, b.moves) and torch.equal(a.scores_after.total, b.scores_after.total) and float(a.sidechain_rmsd_moved.max()) == 0.0
    assert 0 < int((a.flags & 1).sum()) and bool(torch.isfinite(a.trace).all())
    # synthetic tables
    case = chain_case(3, 12, 1, 300, 82)
    cfg = SE.SearchConfig(sidechains=True, replicas=2, cycles=3, iterations=5, seed=12)
    fc = flex_chain_searcher(case, empty_tables(300), cfg)
    rc = chain_searcher(case, cfg)
    y = case[3][None].repeat(3, 1, 1).contiguous()
    sa, sb = fc.advance(fc.start(case[0], y), 3), rc.advance(rc.start(case[0]), 3)
    for k in ("cur_pos", "best_pos"):
        assert torch.equal(bits32(getattr(sa, k)), bits32(getattr(sb, k))), k
    for k in ("cur_e", "best_e", "energy_minimized"):
        assert torch.equal(getattr(sa, k)[:, [0, 1, 3, 5]], getattr(sb, k)), k
    for k in ("best_cycle", "accepted", "trace", "flags", "perturb", "u"):
        assert torch.equal(getattr(sa, k), getattr(sb, k)), k
    # a graph without flexible residues is PoseSearcher's case
    rigid = make_3dpf_complex(seed=2, flexible_sidechains=False, n_lig=12, n_rec=8)
    with pytest.raises(ValueError, match="PoseSearcher"):
        SF.FlexPoseSearcher(rigid, config=cfg)


def test_replica_zero_of_cycle_zero_is_the_joint_minimiser_bit_for_bit():
    g, x, y = flex_fixture()
    x, y = x[:4], y[:4]
    for K in (0, 5):
        fs = SF.FlexPoseSearcher(g, config=SE.SearchConfig(sidechains=True, replicas=3, cycles=2, iterations=K, restraint=0.1, sidechain_restraint=0.1))
        st = fs.advance(fs.start(x, y), 1)
        mz = MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(iterations=K, restraint=0.1, sidechain_restraint=0.1))
        mr = mz.minimize(x, y)
        mov = fs.sc.mov
        assert torch.equal(bits32(st.cur_pos[::3]), bits32(mr.lig_pos)) and torch.equal(bits32(st.best_pos[::3]), bits32(mr.lig_pos))
        assert torch.equal(bits32(st.cur_mov[::3]), bits32(mr.atom_pos[:, mov])) and torch.equal(bits32(st.best_mov[::3]), bits32(mr.atom_pos[:, mov]))
        assert torch.equal(st.cur_e[::3], mr.energy_after) and torch.equal(st.best_e[::3], mr.energy_after) and torch.equal(st.energy_minimized, mr.energy_after)
        assert torch.equal(st.accepted[::3], mr.accepted) and torch.equal(st.trace[0, ::3, 0], mr.energy_before[:, 5])
        assert torch.equal(st.trace[0, ::3, 1], mr.energy_after[:, 5]) and bool((st.flags[0] == 3).all()) and bool((st.best_cycle == 0).all())
        assert not torch.equal(st.trace[0, 1::3, 0], mr.energy_before[:, 5])          # the other replicas started somewhere else
        if K:
            assert int(mr.accepted.sum()) >= 1 and float(mr.sidechain_rmsd_moved.max()) > 0


# ---------------------------------------------------------------------------------------------- 2. bookkeeping and the inequality
def test_decisions_replayed_and_the_exact_inequality_on_the_fixture():
    fs, res, st = fixture_search()
    g, x, y = flex_fixture()
    R, temp = 2, fs.config.temperature
    flags, ecs, ebs, bc, margin = replay(st.trace.numpy(), st.u.numpy(), temp, R)
    assert margin > 1e-9, margin
    assert np.array_equal(flags, st.flags.numpy())
    assert np.array_equal(ebs[-1], st.best_e[:, 5].numpy()) and np.array_equal(ecs[-1], st.cur_e[:, 5].numpy())
    assert np.array_equal(bc, st.best_cycle.numpy())
    rep = select_ref(st.best_e[:, 5].numpy(), R)
    assert np.array_equal(rep, res.replica.numpy())
    q = torch.arange(6) * R + res.replica.long()
    mov = fs.sc.mov
    assert torch.equal(bits32(res.lig_pos), bits32(st.best_pos[q])) and torch.equal(bits32(res.atom_pos[:, mov]), bits32(st.best_mov[q]))
    assert torch.equal(res.energy_after, st.best_e[q]) and torch.equal(res.cycle, st.best_cycle[q])
    assert torch.equal(res.moves, (st.flags[:, q] & 1).sum(0).to(torch.int32))
    # the exact inequality, against the joint minimiser with the same iteration count
    mr = MF.FlexPoseMinimizer(g, config=M.MinimizeConfig(iterations=6)).minimize(x[:6], y[:6])
    assert torch.equal(res.energy_minimized, mr.energy_after) and torch.equal(res.energy_before, mr.energy_before)
    print("E before", [round(float(v), 2) for v in res.energy_before[:, 5]], "\nminimised", [round(float(v), 2) for v in res.energy_minimized[:, 5]],
          "\nsearched", [round(float(v), 2) for v in res.energy_after[:, 5]], "\nside-chain RMSD moved", [round(float(v), 3) for v in res.sidechain_rmsd_moved])
    assert bool((res.energy_after[:, 5] <= res.energy_minimized[:, 5]).all()) and bool((res.energy_minimized[:, 5] <= res.energy_before[:, 5]).all())
    # non-moving atoms come back bit for bit; the moving ones moved; scores_after is the pose against its own searched side chains
    static = torch.ones(y.shape[1], dtype=torch.bool)
    static[mov] = False
    assert torch.equal(bits32(res.atom_pos[:, static]), bits32(y[:6][:, static])) and float(res.sidechain_rmsd_moved.max()) > 0
    sc = fs.scorer.score(res.lig_pos, res.atom_pos)
    assert torch.equal(sc.total, res.scores_after.total) and torch.equal(res.energy_after[:, 0], sc.inter) and torch.equal(res.energy_after[:, 1], sc.intra)
    want = (res.atom_pos[:, mov].double() - y[:6][:, mov].double()).pow(2).sum(-1).mean(-1).sqrt()
    assert torch.allclose(res.sidechain_rmsd_moved.double(), want, atol=1e-5)
    # index() and cpu()
    order = torch.tensor([3, 0, 5])
    part = res.index(order)
    assert torch.equal(part.atom_pos, res.atom_pos[order]) and torch.equal(part.trace, res.trace[:, [6, 7, 0, 1, 10, 11]])
    assert torch.equal(part.scores_after.total, res.scores_after.total[order]) and isinstance(part.cpu(), SF.FlexSearchResult)
    import diffdock_pocket_amd as DP
    assert DP.FlexPoseSearcher is SF.FlexPoseSearcher and DP.FlexSearchResult is SF.FlexSearchResult


def test_a_three_cycle_run_on_synthetic_tables_is_replayed():
    """Side-chain bonds whose axis atoms move themselves, a two-tile receptor: the rules replayed from trace and u."""
    c = F.random_case(3, 37, 1025, 5, 17, seed=5, moving_at=[1023, 1024])
    cfg = SE.SearchConfig(sidechains=True, replicas=2, cycles=3, iterations=3, seed=2)
    fs, x, y = random_flex_searcher(c, 5, cfg)
    starts = []
    st = fs.advance(fs.start(x, y), 3, starts=starts)
    flags, ecs, ebs, bc, margin = replay(st.trace.numpy(), st.u.numpy(), cfg.temperature, 2)
    assert margin > 1e-9 and np.array_equal(flags, st.flags.numpy())
    assert np.array_equal(ebs[-1], st.best_e[:, 5].numpy()) and np.array_equal(ecs[-1], st.cur_e[:, 5].numpy()) and np.array_equal(bc, st.best_cycle.numpy())
    mov = fs.sc.mov
    assert torch.equal(bits32(starts[0][0][::2]), bits32(x)) and torch.equal(bits32(starts[0][1][::2]), bits32(y[:, mov]))
    assert not torch.equal(starts[0][1][1::2], y[:, mov])                   # the other replica's side chains took the random move
    _, _, e, rep, _ = fs.select(st)
    assert bool((e[:, 5] <= st.energy_minimized[:, 5]).all()) and bool((st.energy_minimized[:, 5] <= st.trace[0, ::2, 0]).all())
    assert rep.tolist() == select_ref(st.best_e[:, 5].numpy(), 2).tolist()


# ---------------------------------------------------------------------------------------------- 3. resumption and the random numbers
def test_advance_resumes_and_the_seed_decides_the_numbers():
    fs, _, whole = fixture_search()
    g, x, y = flex_fixture()
    fresh = fs.start(x[:6], y[:6])
    before = {k: getattr(fresh, k).clone() for k in STATE_FIELDS}
    a = fs.advance(fresh, 1)
    same_state(fs.advance(a, 2), whole, "1 + 2")
    same_state(fs.advance(fs.advance(a, 1), 1), whole, "1 + 1 + 1")
    assert all(torch.equal(getattr(fresh, k).nan_to_num(7.0), before[k].nan_to_num(7.0)) for k in STATE_FIELDS) and fresh.cycle == 0
    with pytest.raises(ValueError):
        fs.advance(whole, 1)
    T, n_sc = fs.T, fs.n_sc
    assert n_sc == 4 and fs.n_mov == 7
    p, u = SF.draw_random_numbers_flex(fs.config, 12, T, n_sc)
    assert torch.equal(p, fresh.perturb) and torch.equal(u, fresh.u) and p.shape == (3, 12, 6 + T + n_sc) and u.dtype == torch.float64
    assert bool((u >= 0).all()) and bool((u < 1).all())
    other, _ = SF.draw_random_numbers_flex(SE.SearchConfig(**dict(FIX, seed=1)), 12, T, n_sc)
    assert not torch.equal(other, p)
    # sigma_chi scales only the last n_sc columns, sigma_tor only the torsions
    wide, _ = SF.draw_random_numbers_flex(SE.SearchConfig(**dict(FIX, sigma_chi=0.6)), 12, T, n_sc)
    assert torch.equal(wide[..., :6 + T], p[..., :6 + T]) and torch.equal(wide[..., 6 + T:], 2 * p[..., 6 + T:])
    tor, _ = SF.draw_random_numbers_flex(SE.SearchConfig(**dict(FIX, sigma_tor=0.25)), 12, T, n_sc)
    assert torch.equal(tor[..., 6 + T:], p[..., 6 + T:]) and torch.equal(tor[..., 6:6 + T], 0.5 * p[..., 6:6 + T]) and torch.equal(tor[..., :6], p[..., :6])
    # no side-chain bonds: the numbers of search.py
    p0, u0 = SF.draw_random_numbers_flex(fs.config, 12, T, 0)
    q0, v0 = SE.draw_random_numbers(fs.config, 12, T)
    assert torch.equal(p0, q0) and torch.equal(u0, v0)
    c = SE.SearchConfig()
    assert (c.sidechains, c.sigma_chi, c.sidechain_restraint) == (False, 0.3, 0.0)
    assert list(SE.SearchConfig.__dataclass_fields__)[-3:] == ["sidechains", "sigma_chi", "sidechain_restraint"]
    for bad in (dict(sigma_chi=-1.0), dict(sidechain_restraint=-1.0), dict(replicas=0), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            SF.FlexPoseSearcher(g, config=SE.SearchConfig(**bad))


def test_two_seeds_walk_differently():
    g, x, y = flex_fixture()
    a = SF.FlexPoseSearcher(g, config=SE.SearchConfig(sidechains=True, replicas=2, cycles=1, iterations=2, seed=0))
    b = SF.FlexPoseSearcher(g, config=SE.SearchConfig(sidechains=True, replicas=2, cycles=1, iterations=2, seed=1))
    sa, sb = a.advance(a.start(x[:2], y[:2]), 1), b.advance(b.start(x[:2], y[:2]), 1)
    assert torch.equal(sa.trace[0, ::2], sb.trace[0, ::2]) and not torch.equal(sa.trace[0, 1::2], sb.trace[0, 1::2])


# ---------------------------------------------------------------------------------------------- 4. NaN containment
def test_a_nan_pose_and_a_nan_moving_atom_keep_their_rows_and_touch_no_other():
    g, x, y = flex_fixture()
    fs = SF.FlexPoseSearcher(g, config=SE.SearchConfig(sidechains=True, replicas=2, cycles=2, iterations=3))
    x, y = x[:4], y[:4]
    clean = fs.advance(fs.start(x, y), 2)
    bx, by = x.clone(), y.clone()
    bx[1, 5, 1] = float("nan")
    by[2, int(fs.sc.mov[3]), 0] = float("nan")
    got = fs.advance(fs.start(bx, by), 2)
    mov = fs.sc.mov
    for s in (1, 2):
        for q in (2 * s, 2 * s + 1):
            assert torch.equal(bits32(got.cur_pos[q]), bits32(bx[s])) and torch.equal(bits32(got.best_pos[q]), bits32(bx[s]))
            assert torch.equal(bits32(got.cur_mov[q]), bits32(by[s, mov])) and torch.equal(bits32(got.best_mov[q]), bits32(by[s, mov]))
            assert bool((got.best_e[q] == float("inf")).all()) and bool((got.cur_e[q] == float("inf")).all())
            assert int(got.best_cycle[q]) == -1 and int(got.accepted[q]) == 0 and bool((got.flags[:, q] == 0).all())
            assert bool(torch.isnan(got.trace[:, q]).all())
    keep = [0, 1, 6, 7]
    for k in STATE_FIELDS[:8]:
        assert torch.equal(getattr(got, k)[keep], getattr(clean, k)[keep]), k
    assert torch.equal(got.trace[:, keep], clean.trace[:, keep]) and torch.equal(got.flags[:, keep], clean.flags[:, keep])
    res = fs.result(got)
    assert torch.equal(bits32(res.lig_pos[1]), bits32(bx[1])) and torch.equal(bits32(res.atom_pos[2]), bits32(by[2]))
    assert res.replica[1:3].tolist() == [0, 0] and res.cycle[1:3].tolist() == [-1, -1] and float(res.energy_after[1, 5]) == float("inf")


# ---------------------------------------------------------------------------------------------- 5. ABI
def test_entry_is_declared_exported_built_and_guarded():
    header = open(os.path.join(ROOT, "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ddp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert "ddp_pose_search_flex" in declared and "ddp_pose_search_flex" in L.EXPORTS and set(L.EXPORTS) == declared
    assert "#define DDP_ABI_VERSION 17" in header
    build = __import__("diffdock_pocket_amd.build", fromlist=["SOURCES"])
    csrc = os.path.join(os.path.dirname(build.__file__), "csrc")
    assert "ddp_search_flex.hip" in build.SOURCES and os.path.exists(os.path.join(csrc, "ddp_search_flex.hip"))
    assert os.path.join(csrc, "ddp_minimize_flex_loop.h") in build.HEADERS and os.path.exists(os.path.join(csrc, "ddp_minimize_flex_loop.h"))
    assert _fields_of(header, "ddp_search_flex_args_t") == [f[0] for f in L.SearchFlexArgs._fields_]
    assert L.SearchFlexArgs._fields_[0] == ("flex", L.MinimizeFlexArgs)
    # a ddp_minimize_flex_args_t, 4 int32, 2 doubles, 14 pointers
    assert ctypes.sizeof(L.SearchFlexArgs) == ctypes.sizeof(L.MinimizeFlexArgs) + 16 + 16 + 14 * 8
    assert os.path.exists(L.LIB_PATH), "build the library first (python -m diffdock_pocket_amd.build)"
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.ddp_abi_version.restype = ctypes.c_int
    assert lib.ddp_abi_version() == 17 and hasattr(lib, "ddp_pose_search_flex")
    fn = lib.ddp_pose_search_flex
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    # the host-side checks need no device: they return before any launch.  Pointers only have to be non-NULL for that.
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def rc(**kw):
        f = L.MinimizeFlexArgs(n_samples=2, n=8, m=5, rec_stride=15, n_tor=1, iterations=2, anchor=p, lig_radii=p, lig_flags=p, rec=p, rec_radii=p,
                               rec_flags=p, self_pairs=p, bonds=p, mask_rotate=p, cutoff=8.0, gauss_offset=0.0, gauss_width=0.8,
                               hydrophobic_good=0.0, hydrophobic_bad=2.5, hbond_good=-0.6, hbond_bad=0.0, w_gauss=-0.045, w_repulsion=0.8,
                               w_hydrophobic=-0.035, w_hbond=-0.6, restraint=0.0, grow=2.0, shrink=0.5, step_max=1024.0, rec_anchor=p, n_mov=2,
                               n_sc=1, n_sub=2, mov=p, sc_edge_idx=p, sc_sub=p, sc_map=p, sc_pairs=p, restraint_sc=0.0)
        a = L.SearchFlexArgs(replicas=3, cycles=0, cycle0=0, step_init=1.0, temperature=1.2, perturb=p, u=p, cur_pos=p, cur_mov=p, cur_e=p,
                             best_pos=p, best_mov=p, best_e=p, best_cycle=p, accepted=p, trace=p, flags=p)
        for k, v in kw.items():
            setattr(f if hasattr(f, k) and not hasattr(a, k) else a, k, v)
        a.flex = f
        return fn(ctypes.byref(a), None)

    assert fn(None, None) == -1
    assert rc() == 0 and rc(n_samples=0, replicas=0) == 0                                     # cycles = 0, n_samples = 0: no-ops
    for over in (dict(n=L.DDP_MINIMIZE_MAX_ATOMS + 1), dict(n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1), dict(n_mov=L.DDP_MINIMIZE_FLEX_MAX_MOVING + 1),
                 dict(n_sc=L.DDP_MINIMIZE_FLEX_MAX_BONDS + 1), dict(n=512, n_mov=19, n_sc=0)):
        for cycles in (0, 3):
            assert rc(**{"cycles": cycles, **over}) == -2, over                               # DDP_ELIMIT
    assert L.flex_state_bytes(512, 19, 0) > L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES >= L.flex_state_bytes(512, 18, 0)
    assert rc(n=512, n_mov=18, n_sc=0) == 0
    inf, nan = float("inf"), float("nan")
    for bad in (dict(anchor=None), dict(lig_radii=None), dict(lig_flags=None), dict(rec=None), dict(rec_radii=None), dict(rec_flags=None),
                dict(bonds=None), dict(mask_rotate=None), dict(rec_anchor=None), dict(mov=None), dict(sc_pairs=None), dict(sc_edge_idx=None),
                dict(sc_map=None), dict(sc_sub=None), dict(cutoff=0.0), dict(cutoff=nan), dict(n_samples=-1), dict(n=0), dict(m=-1),
                dict(n_tor=-1), dict(n_mov=-1), dict(n_sc=-1), dict(n_sub=-1), dict(rec_stride=14), dict(rec_stride=0), dict(iterations=-1),
                dict(restraint=-0.1), dict(restraint=nan), dict(restraint_sc=-0.1), dict(restraint_sc=nan), dict(replicas=0), dict(replicas=-2),
                dict(cycles=-1), dict(cycle0=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=inf), dict(temperature=nan),
                dict(step_init=0.0), dict(step_init=-1.0), dict(step_init=nan), dict(perturb=None), dict(u=None), dict(cur_pos=None),
                dict(cur_mov=None), dict(cur_e=None), dict(best_pos=None), dict(best_mov=None), dict(best_e=None), dict(best_cycle=None),
                dict(accepted=None), dict(trace=None), dict(flags=None), dict(n_samples=1 << 30, replicas=4)):
        for cycles in (0, 3):                          # the checks come before the no-op of cycles = 0 and before any launch
            assert rc(**{"cycles": cycles, **bad}) == -1, bad
    assert rc(n_mov=0, n_sc=0, n_sub=0, cur_mov=None, best_mov=None, mov=None, sc_pairs=None, rec_anchor=None) == 0   # nothing moves: not read
    assert bytes(buf) == bytes(64), "a guard wrote through a pointer"


# ---------------------------------------------------------------------------------------------- 6. flags and driver
SMALL = dict(replicas=2, cycles=2, iterations=3)


def test_flags_parse_and_imply_the_search(tmp_path, capsys):
    p = INF._parser()
    a = p.parse_args([])
    assert a.search_sidechains is False and a.search_sigma_chi == 0.3 and a.search_sidechain_restraint == 0.0 and a.search_poses is False
    a = p.parse_args(["--search_sidechains", "--search_sigma_chi", "0.1", "--search_sidechain_restraint", "0.5"])
    assert a.search_sidechains is True and a.search_sigma_chi == 0.1 and a.search_sidechain_restraint == 0.5
    cfg = INF._search_config(a)
    assert isinstance(cfg, SE.SearchConfig) and cfg.sidechains and cfg.sigma_chi == 0.1 and cfg.sidechain_restraint == 0.5
    assert INF._search_config(p.parse_args([])) is None
    plain = INF._search_config(p.parse_args(["--search_poses"]))
    assert plain == SE.SearchConfig() and plain.sidechains is False
    (tmp_path / "model_parameters.yml").write_text("{}\n")
    for bad, msg in ((["--search_sigma_chi", "-1"], "--search_sigma_chi must not be negative"),
                     (["--search_sidechain_restraint", "-1"], "--search_sidechain_restraint must not be negative")):
        with pytest.raises(SystemExit) as e:
            INF.main(["--protein_path", "p.pdb", "--ligand", "l.sdf", "--model_dir", str(tmp_path)] + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err


def test_run_csv_searches_side_chains_of_flexible_rows_only(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)
    plain = _run(str(p), str(tmp_path / "plain"), search_poses=SE.SearchConfig(**SMALL))
    joint = _run(str(p), str(tmp_path / "joint"), search_poses=SE.SearchConfig(sidechains=True, **SMALL))
    new_files = {"searched_sidechains.csv"} | {f"rank{k}_searched_protein.pdb" for k in range(1, 5)}
    for row, (a, b) in enumerate(zip(plain, joint)):
        assert a.skipped is None and b.skipped is None, (a.skipped, b.skipped)
        assert isinstance(a.searched, SE.SearchResult) and torch.equal(a.ligand_pos, b.ligand_pos) and torch.equal(a.order, b.order)
        old = {os.path.basename(f): f for f in a.files}
        new = {os.path.basename(f): f for f in b.files}
        assert set(os.listdir(os.path.dirname(b.files[0]))) == set(new)
        if row == 1:            # the rigid row: nothing new, every file and every tensor as without the flag
            assert isinstance(b.searched, SE.SearchResult) and set(new) == set(old)
            for name, path in old.items():
                assert open(path, "rb").read() == open(new[name], "rb").read(), name
            for k, v in a.searched.__dict__.items():
                w = getattr(b.searched, k)
                if torch.is_tensor(v):
                    assert torch.equal(v.nan_to_num(7.0), w.nan_to_num(7.0)), k
                else:
                    assert torch.equal(v.total, w.total), k
            continue
        sr = b.searched
        assert isinstance(sr, SF.FlexSearchResult) and set(new) - set(old) == new_files and set(old) <= set(new)
        for name, path in old.items():
            if "searched" not in name:
                assert open(path, "rb").read() == open(new[name], "rb").read(), name
        assert torch.equal(sr.lig_pos, b.searched_pos) and sr.atom_pos.shape[0] == 4 and sr.energy_after.shape == (4, 6) and sr.trace.shape == (2, 8, 2)
        assert bool((sr.energy_after[:, 5] <= sr.energy_minimized[:, 5]).all()) and bool((sr.energy_minimized[:, 5] <= sr.energy_before[:, 5]).all())
        rows = _rows(new["searched.csv"])
        from diffdock_pocket_amd import outputs as O
        assert list(rows[0].keys()) == O.SEARCHED_COLUMNS and len(rows) == 4
        sc_rows = _rows(new["searched_sidechains.csv"])
        assert list(sc_rows[0].keys()) == ["rank", "sample", "sc_before", "sc_after", "sidechain_restraint_after", "sidechain_rmsd_moved"]
        for r in range(4):
            assert int(rows[r]["sample"]) == int(sc_rows[r]["sample"]) == int(b.order[r]) and int(sc_rows[r]["rank"]) == r + 1
            for got, val in ((rows[r]["energy_after"], sr.energy_after[r, 5]), (rows[r]["energy_before"], sr.energy_before[r, 5]),
                             (rows[r]["energy_minimized"], sr.energy_minimized[r, 5]), (rows[r]["total_after"], sr.scores_after.total[r]),
                             (sc_rows[r]["sc_before"], sr.energy_before[r, 2]), (sc_rows[r]["sc_after"], sr.energy_after[r, 2]),
                             (sc_rows[r]["sidechain_restraint_after"], sr.energy_after[r, 4])):
                assert abs(float(got) - float(val)) <= 1e-5 * abs(float(val)) + 1e-12
            assert abs(float(sc_rows[r]["sidechain_rmsd_moved"]) - float(sr.sidechain_rmsd_moved[r])) < 1e-4
        # the written receptor carries the searched side chains: its moved atoms are the result's
        moved = [r for r in range(4) if float(sr.sidechain_rmsd_moved[r]) > 1e-3]
        assert moved, "no side chain moved in the miniature"
        k = moved[0]
        sampled = [n for n in old if n.endswith("_protein.pdb") and n.startswith(f"rank{k + 1}_")]
        text = open(new[f"rank{k + 1}_searched_protein.pdb"]).read()
        before = open(old[sampled[0]]).read().splitlines()
        changed = [ln for ln, l0 in zip(text.splitlines(), before) if ln != l0]
        assert changed and len(text.splitlines()) == len(before)
        xyz = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in changed])
        want = sr.atom_pos[k].double().numpy() + np.asarray(b.original_center, dtype=np.float64).reshape(1, 3)
        d = np.linalg.norm(xyz[:, None] - want[None], axis=-1).min(1)
        assert d.max() < 2e-3, d.max()          # (three decimals in the file)
    ranked = _run(str(p), str(tmp_path / "ranked"), rank_by="searched_score", search_poses=SE.SearchConfig(sidechains=True, **SMALL))[0]
    t = ranked.searched.scores_after.total
    assert bool((t[:-1] <= t[1:]).all()) and isinstance(ranked.searched, SF.FlexSearchResult)
    inv_a, inv_b = torch.argsort(joint[0].order), torch.argsort(ranked.order)
    assert torch.equal(bits32(joint[0].searched.atom_pos[inv_a]), bits32(ranked.searched.atom_pos[inv_b]))
