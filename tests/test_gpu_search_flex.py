"""csrc/ddp_search_flex.hip on the device: one cycle of one replica against ddp_pose_minimize_flex and, without side chains, the whole
search against ddp_pose_search, bit for bit; four cycles stage by stage (start states against the CPU maps, the descent against
ddp_pose_minimize_flex from the recorded start states, the decisions replayed in NumPy fp64, the state following the flags);
resumption, determinism and batch independence, bit for bit; the receptor is never written; NaN containment; the flexible 3dpf fixture
against the device minimiser (the exact inequality), the launch-by-launch form and the fall-back above the limits; run_csv on the
device.  TILE = 1024 is DDP_FX_TILE: the receptor is tried on both sides of it, with moving atoms at the tile's edges."""
import os

import numpy as np
import pytest
import torch

import flexmin_ref as F
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd import search_flex as SF
from diffdock_pocket_amd.sampler import modify_conformer, rotate_index_lists
from test_gpu_minimize_flex import TILE, Tables, _raw, device_case, flex_fixture
from test_gpu_search import _search as rigid_search
from test_minimize_cpu import bits32, chain_case
from test_scoring_cpu import CFG
from test_search_cpu import replay
from test_search_flex_cpu import chain_torsions, random_flex_searcher

pytestmark = pytest.mark.gpu
STATE = ("cur_pos", "cur_mov", "cur_e", "best_pos", "best_mov", "best_e", "best_cycle", "accepted")
TEMP = 1.2
EPS32 = 2.0 ** -23
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _numbers(C, rows, T, n_sc, seed, dev):
    p, u = SF.draw_random_numbers_flex(SE.SearchConfig(cycles=C, seed=seed), rows, T, n_sc)
    return p.to(dev), u.to(dev)


def _case(S, n, m, n_mov, n_sc, T, seed, dev, **opt):
    """A flexmin_ref.random_case on the device with a chain torsion table; the sampled state is (x, y)."""
    c = F.random_case(S, n, m, n_mov, n_sc, seed=seed, **opt)
    t = device_case(c, dev)
    bonds, mask = chain_torsions(n, T)
    t["bonds"], t["mask"], t["T"], t["host"] = (bonds.to(dev) if T else None), (mask.to(dev) if T else None), T, c
    return t


def _fresh(rows, n, n_mov, dev):
    """A state filled with a marker: with cycle0 = 0 the kernel must not read it."""
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(cur_pos=torch.full((rows, n, 3), -7.0, device=dev), cur_mov=torch.full((rows, n_mov, 3), -7.0, device=dev),
                cur_e=torch.full((rows, 6), -7.0, **f64), best_pos=torch.full((rows, n, 3), -7.0, device=dev),
                best_mov=torch.full((rows, n_mov, 3), -7.0, device=dev), best_e=torch.full((rows, 6), -7.0, **f64),
                best_cycle=torch.full((rows,), -7, dtype=torch.int32, device=dev), accepted=torch.full((rows,), -7, dtype=torch.int32, device=dev))


def _search(t, R, K, perturb, u, state=None, cycle0=0, starts=False, k=0.0, k_sc=0.0, x=None, y=None):
    """ddp_pose_search_flex on CLONES of the state; returns the state after the call with trace, flags and the starts."""
    x = t["x"] if x is None else x
    y = t["y"] if y is None else y
    S, n, dev = x.shape[0], x.shape[1], x.device
    n_mov = t["tables"]["mov"].shape[0]
    C, rows = u.shape[0], S * R
    st = {key: v.clone() for key, v in (_fresh(rows, n, n_mov, dev) if state is None else state).items() if key in STATE}
    st["trace"] = torch.full((C, rows, 2), -7.0, dtype=torch.float64, device=dev)
    st["flags"] = torch.full((C, rows), 77, dtype=torch.uint8, device=dev)
    st["starts"] = torch.full((C, rows, n, 3), -7.0, device=dev) if starts else None
    st["starts_mov"] = torch.full((C, rows, n_mov, 3), -7.0, device=dev) if starts else None
    LA.pose_search_flex(x, t["lig_r"], t["lig_f"], y, t["rec_r"], t["rec_f"], CFG, t["pairs"], t["bonds"], t["mask"], t["tables"], R, cycle0,
                        perturb, u, st["cur_pos"], st["cur_mov"], st["cur_e"], st["best_pos"], st["best_mov"], st["best_e"], st["best_cycle"],
                        st["accepted"], st["trace"], st["flags"], K, TEMP, restraint=k, restraint_sc=k_sc, starts=st["starts"],
                        starts_mov=st["starts_mov"])
    return st


def _same(a, b, what, keys=STATE + ("trace", "flags")):
    for key in keys:
        assert torch.equal(_bits(a[key]), _bits(b[key])), f"{what}: {key}"


# ---------------------------------------------------------------------------------------------- 1. one cycle, one replica
@pytest.mark.parametrize("shape", [(3, 5, TILE - 1, 4, 1, 2, 1059, {}), (3, 37, TILE + 1, 5, 17, 5, 1093, dict(moving_at=[TILE - 1, TILE])),
                                   (1, 1, 1, 1, 0, 0, 1, {})],
                         ids=lambda s: "S{}-n{}-m{}-mov{}-sc{}".format(*s[:5]))
def test_one_cycle_of_one_replica_is_ddp_pose_minimize_flex(shape):
    dev = _dev()
    S, n, m, n_mov, n_sc, T, seed, opt = shape      # (the seeds: at each the CPU form accepts a trial within 7 iterations)
    t = _case(S, n, m, n_mov, n_sc, T, seed, dev, **opt)
    mov = t["tables"]["mov"].long()
    p, u = _numbers(1, S, T, n_sc, 5, dev)
    anchored = dict(t, x0=t["x"], y0=t["y"])          # the sampled state is the anchor
    for K in (0, 7):
        st = _search(t, 1, K, p, u, k=0.1, k_sc=0.1)
        out = _raw(anchored, K, 0.1, 0.1, t["bonds"], t["mask"])
        torch.cuda.synchronize()
        for key in ("cur_pos", "best_pos"):
            assert torch.equal(_bits(st[key]), _bits(out["x"])), (key, K)
        for key in ("cur_mov", "best_mov"):
            assert torch.equal(_bits(st[key]), _bits(out["y"][:, mov])), (key, K)
        assert torch.equal(_bits(st["cur_e"]), _bits(out["e1"])) and torch.equal(_bits(st["best_e"]), _bits(out["e1"])), K
        assert torch.equal(st["accepted"], out["acc"]) and bool((st["best_cycle"] == 0).all()) and bool((st["flags"] == 3).all())
        assert torch.equal(_bits(st["trace"][0, :, 0]), _bits(out["e0"][:, 5])) and torch.equal(_bits(st["trace"][0, :, 1]), _bits(out["e1"][:, 5]))
        assert bool(torch.isfinite(out["e1"]).all())
        if K == 7:
            assert int(out["acc"].sum()) >= 1, "the case never accepts: it checks nothing of the descent"


# ---------------------------------------------------------------------------------------------- 2. no side chains
@pytest.mark.parametrize("n,T", [(12, 1), (37, 5)])
def test_without_side_chains_it_is_ddp_pose_search_bit_for_bit(n, T):
    dev = _dev()
    S = R = C = 3
    K, m = 5, TILE + 1
    case = [a.to(dev) for a in chain_case(S, n, T, m, 40 + n)]
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = case
    y = rec[None].repeat(S, 1, 1).contiguous()
    empty = LA.flex_tables(Tables(dict(mov=np.zeros(0, np.int64), sc_pairs=np.zeros((0, m), np.uint8), edge=np.zeros((0, 2), np.int64),
                                       mapping=np.zeros((0, 2), np.int64), sub=np.zeros(0, np.int64))), m, dev)
    t = dict(x=x, y=y, lig_r=lig_r, lig_f=lig_f, rec_r=rec_r, rec_f=rec_f, pairs=pairs, tables=empty, bonds=bonds, mask=mask)
    p, u = _numbers(C, S * R, T, 0, 6, dev)
    a = _search(t, R, K, p, u, k=0.05, k_sc=0.4)
    b = rigid_search(case, R, K, p, u, k=0.05)
    torch.cuda.synchronize()
    for key in ("cur_pos", "best_pos", "best_cycle", "accepted", "trace", "flags"):
        assert torch.equal(_bits(a[key]), _bits(b[key])), key
    for key in ("cur_e", "best_e"):
        assert torch.equal(_bits(a[key][:, [0, 1, 5]]), _bits(b[key][:, [0, 1, 3]])), key
    assert int((a["flags"] & 1).sum()) >= S * R and int(a["accepted"].sum()) >= 1 and bool(torch.isfinite(a["best_e"]).all())


# ---------------------------------------------------------------------------------------------- 3. stage by stage
STAGE_SEED = 0        # of the random numbers; chosen with the CPU form (the definition) so that it alone meets the two conditions of (c)


def test_four_cycles_stage_by_stage():
    """S = 3, R = 3, K = 5, (n, m, n_mov, n_sc) = (37, 1025, 5, 17), four 1-cycle calls with the start states recorded and the state read
    between the calls.
    The bound of the start side chains against the fp64 restatement: bond j turns an atom p about the axis a_j = y_u - y_v through y_v in
    fp32.  Normalising the axis, sin and cos, the nine products of the matrix, the three-term dot products and the shift back each cost
    at most a few ulp of the numbers they handle, which are at most L_j + |y_v| <= 2 scale (L_j: the longest lever |p - y_v| of the
    bond, scale: the largest |coordinate|): at most 16 EPS32 scale per bond and atom.  An error e already in the axis atoms tilts the
    axis by at most 2 e / |a_j| and moves a turned atom by at most 2 e L_j / |a_j|; to first order the contributions of the at most
    n_sc bonds that turn an atom or its axes add:
        bound = n_sc * 16 * EPS32 * scale * (1 + 2 max_j L_j / |a_j|),  EPS32 = 2^-23,
    with L_j and |a_j| read off the fp64 restatement's own states."""
    dev = _dev()
    S, R, K, n, m, n_mov, n_sc, T = 3, 3, 5, 37, TILE + 1, 5, 17, 5
    t = _case(S, n, m, n_mov, n_sc, T, 77, dev, moving_at=[TILE - 1, TILE])
    c = t["host"]
    mov = t["tables"]["mov"].long()
    rows = S * R
    p, u = _numbers(4, rows, T, n_sc, STAGE_SEED, dev)
    x0, y0 = t["x"], t["y"]
    xr, yr = x0.repeat_interleave(R, 0), y0.repeat_interleave(R, 0)
    per_row = dict(t, x0=xr, y0=yr)
    bonds, mask = chain_torsions(n, T)
    rot_idx = rotate_index_lists(mask.bool())
    state, margin_all, moves, stays = None, np.inf, 0, 0
    for cyc in range(4):
        before = state
        state = _search(t, R, K, p[cyc:cyc + 1], u[cyc:cyc + 1], state, cycle0=cyc, starts=True)
        torch.cuda.synchronize()
        cur_x = xr if before is None else before["cur_pos"]
        cur_m = yr[:, mov] if before is None else before["cur_mov"]
        # a. the start states
        start, start_m = state["starts"][0], state["starts_mov"][0]
        want = modify_conformer(cur_x.cpu(), p[cyc, :, 0:3].cpu(), p[cyc, :, 3:6].cpu(), p[cyc, :, 6:6 + T].cpu(), bonds.long(), rot_idx)
        first = torch.zeros(rows, dtype=torch.bool)
        if cyc == 0:
            first[::R] = True
            assert torch.equal(_bits(start[::R]), _bits(x0)) and torch.equal(_bits(start_m[::R]), _bits(y0[:, mov])), "replica 0 does not start at the sampled state"
        scale = float(want.abs().max())
        worst = float((start.cpu()[~first].double() - want[~first].double()).abs().max())
        print(f"cycle {cyc}: start poses off the CPU pose map by {worst:.2e} (bound {2e-5 * scale:.2e})")
        assert worst <= 2e-5 * scale
        yc = yr.clone()
        yc[:, mov] = cur_m
        yc, chi = yc.cpu().numpy(), p[cyc, :, 6 + T:].cpu().numpy()
        worst_sc, worst_bound = 0.0, 0.0
        for q in range(rows):
            if first[q]:
                continue
            ref = F.apply_sidechains(yc[q], c["edge"], c["sub"], c["mapping"], chi[q].astype(np.float64))
            ratio = 0.0
            for j in range(n_sc):
                uu, vv = int(c["edge"][j][0]), int(c["edge"][j][1])
                idx = c["sub"][int(c["mapping"][j][0]):int(c["mapping"][j][1])]
                for geom in (yc[q].astype(np.float64), ref):
                    ratio = max(ratio, float(np.linalg.norm(geom[idx] - geom[vv], axis=-1).max() / np.linalg.norm(geom[uu] - geom[vv])))
            bound = n_sc * 16 * EPS32 * float(np.abs(ref).max()) * (1.0 + 2.0 * ratio)
            err = float(np.abs(start_m[q].cpu().numpy().astype(np.float64) - ref[c["mov"]]).max())
            if err / bound > worst_sc / max(worst_bound, 1e-300):
                worst_sc, worst_bound = err, bound
            assert err <= bound, (cyc, q, err, bound)
        print(f"cycle {cyc}: start side chains off the fp64 map by {worst_sc:.2e} (bound {worst_bound:.2e})")
        # b. the descent is ddp_pose_minimize_flex from the start state, anchored at the sampled state
        ys = yr.clone()
        ys[:, mov] = start_m
        out = _raw(per_row, K, 0.0, 0.0, t["bonds"], t["mask"], x=start, y=ys)
        torch.cuda.synchronize()
        assert torch.equal(_bits(state["trace"][0, :, 0]), _bits(out["e0"][:, 5])) and torch.equal(_bits(state["trace"][0, :, 1]), _bits(out["e1"][:, 5]))
        flags = state["flags"][0].cpu()
        move, improved = (flags & 1).bool(), (flags & 2).bool()
        # d. the state follows the flags by bits; rows that did not move or improve keep their bits
        best_x = xr if before is None else before["best_pos"]
        best_m = yr[:, mov] if before is None else before["best_mov"]
        for got, new, old, sel in ((state["cur_pos"], out["x"], cur_x, move), (state["cur_mov"], out["y"][:, mov], cur_m, move),
                                   (state["best_pos"], out["x"], best_x, improved), (state["best_mov"], out["y"][:, mov], best_m, improved)):
            assert torch.equal(_bits(got.cpu()[sel]), _bits(new.cpu()[sel])) and torch.equal(_bits(got.cpu()[~sel]), _bits(old.cpu()[~sel]))
        acc_before = 0 if before is None else before["accepted"]
        assert torch.equal(state["accepted"], acc_before + out["acc"])
        # c. the decisions, replayed in NumPy fp64
        ec0 = None if before is None else before["cur_e"][:, 5].cpu().numpy()
        eb0 = None if before is None else before["best_e"][:, 5].cpu().numpy()
        bc0 = None if before is None else before["best_cycle"].cpu().numpy()
        f, ecs, ebs, bc, margin = replay(state["trace"].cpu().numpy(), u[cyc:cyc + 1].cpu().numpy(), TEMP, R, ec0, eb0, bc0, cyc)
        margin_all = min(margin_all, margin)
        assert margin > 1e-9, f"cycle {cyc}: a decision lies within 1e-9 of its random number: not comparable between two exp"
        assert np.array_equal(f[0], flags.numpy()), (cyc, f[0], flags)
        moves, stays = moves + int(move.sum()), stays + int((~move).sum())
        assert np.array_equal(ecs[-1], state["cur_e"][:, 5].cpu().numpy()) and np.array_equal(ebs[-1], state["best_e"][:, 5].cpu().numpy())
        assert np.array_equal(bc, state["best_cycle"].cpu().numpy())
        inf6 = torch.full_like(out["e1"], float("inf"))
        eb_before, ec_before = (inf6, inf6) if before is None else (before["best_e"], before["cur_e"])
        assert torch.equal(_bits(state["best_e"]), _bits(torch.where(improved.to(dev)[:, None], out["e1"], eb_before)))
        assert torch.equal(_bits(state["cur_e"]), _bits(torch.where(move.to(dev)[:, None], out["e1"], ec_before)))
    print(f"decisions: {moves} moves, {stays} stays, smallest margin {margin_all:.3e}")
    assert moves > rows and stays > 0, "the case does not exercise both outcomes"


# ---------------------------------------------------------------------------------------------- 4. resumption, determinism, independence
def _whole(n_sc, dev):
    """(case, numbers, the 4-cycle run) of the three shapes of test 4, once per shape."""
    if n_sc not in _CACHE:
        S, n, m, n_mov, T, opt = {0: (3, 5, TILE - 1, 4, 2, {}), 1: (3, 5, TILE - 1, 4, 2, {}),
                                  17: (3, 37, TILE + 1, 5, 5, dict(moving_at=[TILE - 1, TILE]))}[n_sc]
        t = _case(S, n, m, n_mov, n_sc, T, 23 + n_sc, dev, **opt)
        p, u = _numbers(4, S * 3, T, n_sc, 9, dev)
        y_before = t["y"].clone()
        _CACHE[n_sc] = (t, p, u, _search(t, 3, 5, p, u, k=0.05, k_sc=0.05), y_before)
    return _CACHE[n_sc]


@pytest.mark.parametrize("n_sc", [0, 1, 17])
def test_split_calls_repeated_launches_and_single_poses_give_the_same_bits(n_sc):
    dev = _dev()
    S, R, K = 3, 3, 5
    t, p, u, whole, _ = _whole(n_sc, dev)
    kw = dict(k=0.05, k_sc=0.05)
    again = _search(t, R, K, p, u, **kw)
    _same(whole, again, "two launches")
    a = _search(t, R, K, p[:2], u[:2], **kw)
    b = _search(t, R, K, p[2:], u[2:], a, cycle0=2, **kw)
    _same(whole, b, "2 + 2", STATE)
    assert torch.equal(_bits(torch.cat([a["trace"], b["trace"]])), _bits(whole["trace"])) and torch.equal(torch.cat([a["flags"], b["flags"]]), whole["flags"])
    for s in range(S):
        one = _search(t, R, K, p[:, s * R:(s + 1) * R].contiguous(), u[:, s * R:(s + 1) * R].contiguous(), x=t["x"][s:s + 1].contiguous(),
                      y=t["y"][s:s + 1].contiguous(), **kw)
        for key in STATE:
            assert torch.equal(_bits(one[key]), _bits(whole[key][s * R:(s + 1) * R])), (s, key)
        assert torch.equal(_bits(one["trace"]), _bits(whole["trace"][:, s * R:(s + 1) * R])) and torch.equal(one["flags"], whole["flags"][:, s * R:(s + 1) * R])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole["best_e"]).all()) and int(whole["accepted"].sum()) >= 1 and int((whole["flags"] & 1).sum()) >= S * R


# ---------------------------------------------------------------------------------------------- 5. the receptor is read only
def test_the_receptor_is_never_written():
    dev = _dev()
    t, p, u, whole, y_before = _whole(17, dev)
    torch.cuda.synchronize()
    mov = t["tables"]["mov"].long()
    assert torch.equal(_bits(t["y"]), _bits(y_before)), "rec changed"
    assert int((whole["flags"] & 1).sum()) >= 9, "a row never moved: nothing could have been written"
    assert not torch.equal(_bits(whole["best_mov"]), _bits(y_before[:, mov].repeat_interleave(3, 0))), "no side chain moved"


# ---------------------------------------------------------------------------------------------- 6. NaN containment
def test_a_nan_pose_and_a_nan_moving_atom_write_only_the_fresh_state():
    dev = _dev()
    S, R, K, n, m, n_mov, n_sc, T = 3, 2, 4, 37, TILE + 1, 5, 17, 5
    t = _case(S, n, m, n_mov, n_sc, T, 17, dev, moving_at=[TILE - 1, TILE])
    mov = t["tables"]["mov"].long()
    p, u = _numbers(3, S * R, T, n_sc, 4, dev)
    bx, by = t["x"].clone(), t["y"].clone()
    bx[1, 5, 1] = float("nan")
    by[2, int(mov[3]), 2] = float("nan")
    got = _search(t, R, K, p, u, x=bx, y=by)
    solo = _search(t, R, K, p[:, :R].contiguous(), u[:, :R].contiguous(), x=t["x"][:1].contiguous(), y=t["y"][:1].contiguous())
    torch.cuda.synchronize()
    for s in (1, 2):
        for q in (R * s, R * s + 1):
            assert torch.equal(_bits(got["cur_pos"][q]), _bits(bx[s])) and torch.equal(_bits(got["best_pos"][q]), _bits(bx[s]))
            assert torch.equal(_bits(got["cur_mov"][q]), _bits(by[s, mov])) and torch.equal(_bits(got["best_mov"][q]), _bits(by[s, mov]))
            assert bool((got["best_e"][q] == float("inf")).all()) and bool((got["cur_e"][q] == float("inf")).all())
            assert int(got["best_cycle"][q]) == -1 and int(got["accepted"][q]) == 0 and bool((got["flags"][:, q] == 0).all())
            assert bool(torch.isnan(got["trace"][:, q]).all())
    for key in STATE:
        assert torch.equal(_bits(got[key][:R]), _bits(solo[key])), key
    assert torch.equal(_bits(got["trace"][:, :R]), _bits(solo["trace"])) and torch.equal(got["flags"][:, :R], solo["flags"])
    assert bool(torch.isfinite(solo["best_e"]).all())


# ---------------------------------------------------------------------------------------------- 7. the fixture and the forms
def test_the_fixture_is_never_worse_than_the_device_joint_minimiser():
    """16 poses of the flexible 3dpf fixture, R = 3, C = 3, K = 10 (48 rows): the exact inequality; energy_minimized is the device
    FlexPoseMinimizer at 10 iterations, by bits; the side chains move; the launch-by-launch form obeys the inequality too."""
    dev = _dev()
    g, x, y = flex_fixture()
    cfg = SE.SearchConfig(sidechains=True, replicas=3, cycles=3, iterations=10)
    fs = SF.FlexPoseSearcher(g, dev, config=cfg)
    xd, yd = x.to(dev), y.to(dev)
    res = fs.search(xd, yd)
    mres = MF.FlexPoseMinimizer(g, dev, config=M.MinimizeConfig(iterations=10)).minimize(xd, yd)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y) and res.lig_pos.is_cuda and res.trace.shape == (3, 48, 2)
    assert torch.equal(_bits(res.energy_minimized), _bits(mres.energy_after)) and torch.equal(_bits(res.energy_before), _bits(mres.energy_before))
    h = res.cpu()
    print("E before", [round(float(v), 2) for v in h.energy_before[:, 5]], "\nminimised", [round(float(v), 2) for v in h.energy_minimized[:, 5]],
          "\nsearched", [round(float(v), 2) for v in h.energy_after[:, 5]], "\nreplica", h.replica.tolist(), "cycle", h.cycle.tolist(),
          "\nside-chain RMSD moved", [round(float(v), 3) for v in h.sidechain_rmsd_moved])
    assert bool((h.energy_after[:, 5] <= h.energy_minimized[:, 5]).all()) and bool((h.energy_minimized[:, 5] <= h.energy_before[:, 5]).all())
    assert float(h.sidechain_rmsd_moved.max()) > 0
    mov = fs.sc.mov
    static = torch.ones(y.shape[1], dtype=torch.bool)
    static[mov] = False
    assert torch.equal(bits32(h.atom_pos[:, static]), bits32(y[:, static]))
    sc = fs.scorer.score(res.lig_pos, res.atom_pos).cpu()
    assert bool(((h.energy_after[:, 0] - sc.inter).abs() <= 1e-9 * sc.inter.abs() + 1e-12).all())
    torch.cuda.set_sync_debug_mode("error")          # neither device form synchronises
    try:
        res2 = fs.search(xd, yd)
        slow = fs.search(xd, yd, fused=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(res2.lig_pos), _bits(res.lig_pos)) and torch.equal(_bits(res2.atom_pos), _bits(res.atom_pos))
    assert torch.equal(_bits(res2.energy_after), _bits(res.energy_after))
    slow = slow.cpu()
    assert bool((slow.energy_after[:, 5] <= slow.energy_minimized[:, 5]).all()) and bool((slow.energy_minimized[:, 5] <= slow.energy_before[:, 5]).all())
    assert torch.equal(_bits(slow.energy_before), _bits(h.energy_before)) and float(slow.sidechain_rmsd_moved.max()) > 0


def test_above_the_limits_the_class_warns_once_and_takes_the_pytorch_form():
    dev = _dev()
    n_mov = L.DDP_MINIMIZE_FLEX_MAX_MOVING + 1
    c = F.random_case(2, 5, n_mov + 40, n_mov, 1, seed=3)
    cfg = SE.SearchConfig(sidechains=True, replicas=2, cycles=2, iterations=1, seed=1)
    fs, x, y = random_flex_searcher(c, 2, cfg, dev)
    assert not fs.minimizer.fused_available()
    M._warned.clear()
    with pytest.warns(UserWarning, match="FlexPoseSearcher.*DDP_MINIMIZE_FLEX_MAX_MOVING"):
        got = fs.advance(fs.start(x.to(dev), y.to(dev)), 2)
    cpu, _, _ = random_flex_searcher(c, 2, cfg)
    want = cpu.advance(cpu.start(x, y), 2)
    torch.cuda.synchronize()
    assert got.cur_pos.is_cuda and got.cycle == 2
    for key in STATE + ("trace", "flags"):
        assert torch.equal(_bits(getattr(got, key).cpu()), _bits(getattr(want, key))), key
    _, _, e, _, _ = fs.select(got)
    assert bool((e[:, 5] <= got.energy_minimized[:, 5]).all()) and bool((got.energy_minimized[:, 5] <= got.trace[0, ::2, 0]).all())
    with pytest.raises(L.DdpError, match="DDP_MINIMIZE_FLEX_MAX_MOVING"):
        t = device_case(c, dev)
        t["bonds"], t["mask"] = None, None
        _search(t, 1, 1, *_numbers(1, 2, 0, 1, 0, dev))


# ---------------------------------------------------------------------------------------------- 8. the driver on the device
def test_run_csv_searches_side_chains_on_the_device(tmp_path):
    from test_gpu_trajectory import GOLDEN, _model_dir
    dev = _dev()
    model_dir = _model_dir(tmp_path, True)
    model, margs, sigma = INF._load_model(model_dir, "best_ema_inference_epoch_model.pt", dev)
    pdb, sdf = os.path.join(GOLDEN, "3dpf_protein.pdb"), os.path.join(GOLDEN, "3dpf_ligand.sdf")
    csv_path = tmp_path / "one.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                        f"3dpf,{pdb},{sdf},,,,A:160-A:193-A:197\n")
    gk = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction", "pocket_buffer",
                                         "pocket_cutoff")}
    gk["flexdist"] = float(margs.flexdist)
    from diffdock_pocket_amd.sampler import SamplerConfig
    cfg = SamplerConfig(inference_steps=4, sigma=sigma, flexible_sidechains=True)
    res = INF.run_csv(str(csv_path), model, dev, samples_per_complex=3, inference_steps=4, seed=7, sampler_cfg=cfg, graph_kwargs=gk,
                      allow_zero_esm=True, out_dir=str(tmp_path / "out"),
                      search_poses=SE.SearchConfig(sidechains=True, replicas=3, cycles=2, iterations=3))[0]
    assert res.skipped is None, res.skipped
    sr = res.searched
    assert isinstance(sr, SF.FlexSearchResult) and not sr.lig_pos.is_cuda and sr.lig_pos.shape == res.ligand_pos.shape
    assert torch.equal(sr.lig_pos, res.searched_pos) and sr.trace.shape == (2, 9, 2) and sr.energy_after.shape == (3, 6)
    assert bool(torch.isfinite(sr.energy_after).all()) and bool(torch.isfinite(sr.lig_pos).all()) and bool(torch.isfinite(sr.atom_pos).all())
    assert bool((sr.energy_after[:, 5] <= sr.energy_minimized[:, 5]).all()) and bool((sr.energy_minimized[:, 5] <= sr.energy_before[:, 5]).all())
    names = {os.path.basename(f) for f in res.files}
    assert {"searched.csv", "searched_sidechains.csv"} | {f"rank{k}_searched.sdf" for k in (1, 2, 3)} | \
        {f"rank{k}_searched_protein.pdb" for k in (1, 2, 3)} <= names
    assert names == set(os.listdir(os.path.dirname(res.files[0])))
    torch.cuda.synchronize()
