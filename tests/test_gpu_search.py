"""csrc/ddp_search.hip on the device: one cycle of one replica against ddp_pose_minimize, bit for bit; four cycles stage by stage (start
poses against the CPU pose map, the descent against ddp_pose_minimize from the recorded start poses, the decisions replayed in NumPy
fp64, the running best); resumption, determinism and batch independence, bit for bit; forced Metropolis decisions; the selection entry
on crafted energies; NaN containment; the 3dpf fixture against the device minimiser (the exact inequality) and an independent score;
the limits and the launch-by-launch form; run_csv on the device."""
import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd.sampler import modify_conformer, rotate_index_lists
from test_minimize_cpu import chain_case, tiled_graph
from test_scoring_cpu import CFG, fixture_3dpf, perturbed_poses
from test_search_cpu import U_HIGH, chain_searcher, replay, select_ref

pytestmark = pytest.mark.gpu
STATE = ("cur_pos", "cur_e", "best_pos", "best_e", "best_cycle", "accepted")
TEMP = 1.2


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _numbers(C, rows, T, seed, dev):
    p, u = SE.draw_random_numbers(SE.SearchConfig(cycles=C, seed=seed), rows, T)
    return p.to(dev), u.to(dev)


def _fresh(rows, n, dev):
    """A state filled with a marker: with cycle0 = 0 the kernel must not read it."""
    return dict(cur_pos=torch.full((rows, n, 3), -7.0, device=dev), cur_e=torch.full((rows, 4), -7.0, dtype=torch.float64, device=dev),
                best_pos=torch.full((rows, n, 3), -7.0, device=dev), best_e=torch.full((rows, 4), -7.0, dtype=torch.float64, device=dev),
                best_cycle=torch.full((rows,), -7, dtype=torch.int32, device=dev), accepted=torch.full((rows,), -7, dtype=torch.int32, device=dev))


def _search(case, R, K, perturb, u, state=None, cycle0=0, starts=False, k=0.0, x0=None):
    """ddp_pose_search on CLONES of the state; returns the state after the call with trace, flags and starts."""
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = case
    x0 = x if x0 is None else x0
    S, n, dev, T = x0.shape[0], x0.shape[1], x0.device, bonds.shape[0]
    C, rows = u.shape[0], S * R
    st = {key: v.clone() for key, v in (_fresh(rows, n, dev) if state is None else state).items() if key in STATE}
    st["trace"] = torch.full((C, rows, 2), -7.0, dtype=torch.float64, device=dev)
    st["flags"] = torch.full((C, rows), 77, dtype=torch.uint8, device=dev)
    st["starts"] = torch.full((C, rows, n, 3), -7.0, device=dev) if starts else None
    LA.pose_search(x0, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, bonds if T else None, mask if T else None, R, cycle0, perturb, u,
                   st["cur_pos"], st["cur_e"], st["best_pos"], st["best_e"], st["best_cycle"], st["accepted"], st["trace"], st["flags"], K, TEMP,
                   restraint=k, starts=st["starts"])
    return st


def _minimize(case, x, anchor, K, k=0.0):
    """ddp_pose_minimize from x with step 1: (x, accepted, e_in, e_out)."""
    _, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = case
    S, dev, T = x.shape[0], x.device, bonds.shape[0]
    x = x.clone()
    step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    e0, e1 = torch.empty(S, 4, dtype=torch.float64, device=dev), torch.empty(S, 4, dtype=torch.float64, device=dev)
    LA.pose_minimize(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, bonds if T else None, mask if T else None, step, acc, e0, e1, K,
                     restraint=k)
    return x, acc, e0, e1


def _same(a, b, what, keys=STATE + ("trace", "flags")):
    for key in keys:
        assert torch.equal(_bits(a[key]), _bits(b[key])), f"{what}: {key}"


# ---------------------------------------------------------------------------------------------- 1. one cycle, one replica
@pytest.mark.parametrize("n,T", [(1, 0), (12, 0), (12, 1), (12, 5), (37, 0), (37, 1), (37, 5)])
def test_one_cycle_of_one_replica_is_ddp_pose_minimize(n, T):
    dev = _dev()
    for m in (0, 1025):
        case = [a.to(dev) for a in chain_case(3, n, T, m, 11 + n + T + m)]
        p, u = _numbers(1, 3, T, 5, dev)
        for K in (0, 7):
            st = _search(case, 1, K, p, u, k=0.1)
            xm, acc, e0, e1 = _minimize(case, case[0], case[0], K, k=0.1)
            torch.cuda.synchronize()
            for key in ("cur_pos", "best_pos"):
                assert torch.equal(_bits(st[key]), _bits(xm)), (key, m, K)
            assert torch.equal(_bits(st["cur_e"]), _bits(e1)) and torch.equal(_bits(st["best_e"]), _bits(e1)), (m, K)
            assert torch.equal(st["accepted"], acc) and bool((st["best_cycle"] == 0).all()) and bool((st["flags"] == 3).all())
            assert torch.equal(_bits(st["trace"][0, :, 0]), _bits(e0[:, 3])) and torch.equal(_bits(st["trace"][0, :, 1]), _bits(e1[:, 3]))
            if K == 7 and m > 0:         # (without a receptor a rigid ligand has nothing to descend: intra does not see a rigid move)
                assert int(acc.sum()) >= 1, "the case never accepts: it checks nothing of the descent"


# ---------------------------------------------------------------------------------------------- 2. stage by stage
def test_four_cycles_stage_by_stage():
    """S = 3, R = 3, K = 5, four 1-cycle calls with the start poses recorded and the state read between the calls."""
    dev = _dev()
    S, R, K, n, T = 3, 3, 5, 37, 5
    host = chain_case(S, n, T, 300, 91)
    case = [a.to(dev) for a in host]
    x0 = case[0]
    rows = S * R
    p, u = _numbers(4, rows, T, 3, dev)
    anchor = x0.repeat_interleave(R, 0)
    rot_idx = rotate_index_lists(host[8].bool())
    state, margin_all, moves, stays = None, np.inf, 0, 0
    for c in range(4):
        before = state
        state = _search(case, R, K, p[c:c + 1], u[c:c + 1], state, cycle0=c, starts=True)
        torch.cuda.synchronize()
        cur_before = anchor if before is None else before["cur_pos"]
        # a. the start poses
        start = state["starts"][0]
        want = modify_conformer(cur_before.cpu(), p[c, :, 0:3].cpu(), p[c, :, 3:6].cpu(), p[c, :, 6:].cpu(), host[7].long(), rot_idx)
        first = torch.zeros(rows, dtype=torch.bool)
        if c == 0:
            first[::R] = True
            assert torch.equal(_bits(start[::R]), _bits(x0)), "replica 0 does not start at the sampled pose"
        scale = float(want.abs().max())
        worst = float((start.cpu()[~first].double() - want[~first].double()).abs().max())
        print(f"cycle {c}: start poses off the CPU pose map by {worst:.2e} (bound {2e-5 * scale:.2e})")
        assert worst <= 2e-5 * scale
        # b. the descent is ddp_pose_minimize from the start pose, anchored at the sampled pose
        xm, acc, e0, e1 = _minimize(case, start, anchor, K)
        torch.cuda.synchronize()
        assert torch.equal(_bits(state["trace"][0, :, 0]), _bits(e0[:, 3])) and torch.equal(_bits(state["trace"][0, :, 1]), _bits(e1[:, 3]))
        flags = state["flags"][0].cpu()
        move, improved = (flags & 1).bool(), (flags & 2).bool()
        assert torch.equal(_bits(state["cur_pos"].cpu()[move]), _bits(xm.cpu()[move]))
        assert torch.equal(_bits(state["cur_pos"].cpu()[~move]), _bits(cur_before.cpu()[~move]))
        assert torch.equal(_bits(state["best_pos"].cpu()[improved]), _bits(xm.cpu()[improved]))
        acc_before = 0 if before is None else before["accepted"]
        assert torch.equal(state["accepted"], acc_before + acc)
        # c. the decisions, replayed in NumPy fp64
        ec0 = None if before is None else before["cur_e"][:, 3].cpu().numpy()
        eb0 = None if before is None else before["best_e"][:, 3].cpu().numpy()
        bc0 = None if before is None else before["best_cycle"].cpu().numpy()
        f, ecs, ebs, bc, margin = replay(state["trace"].cpu().numpy(), u[c:c + 1].cpu().numpy(), TEMP, R, ec0, eb0, bc0, c)
        margin_all = min(margin_all, margin)
        assert margin > 1e-9, f"cycle {c}: a decision lies within 1e-9 of its random number: not comparable between two exp"
        assert np.array_equal(f[0], flags.numpy()), (c, f[0], flags)
        moves, stays = moves + int(move.sum()), stays + int((~move).sum())
        # d. the energies of the state follow
        assert np.array_equal(ecs[-1], state["cur_e"][:, 3].cpu().numpy()) and np.array_equal(ebs[-1], state["best_e"][:, 3].cpu().numpy())
        assert np.array_equal(bc, state["best_cycle"].cpu().numpy())
        eb_before = torch.full_like(e1, float("inf")) if before is None else before["best_e"]
        ec_before = torch.full_like(e1, float("inf")) if before is None else before["cur_e"]
        assert torch.equal(_bits(state["best_e"]), _bits(torch.where(improved.to(dev)[:, None], e1, eb_before)))
        assert torch.equal(_bits(state["cur_e"]), _bits(torch.where(move.to(dev)[:, None], e1, ec_before)))
    print(f"decisions: {moves} moves, {stays} stays, smallest margin {margin_all:.3e}")
    assert moves > rows and stays > 0, "the case does not exercise both outcomes"


# ---------------------------------------------------------------------------------------------- 3. resumption, determinism, independence
@pytest.mark.parametrize("n,T", [(12, 1), (37, 5)])
def test_split_calls_repeated_launches_and_single_poses_give_the_same_bits(n, T):
    dev = _dev()
    S, R, K = 3, 3, 5
    case = [a.to(dev) for a in chain_case(S, n, T, 1025, 23 + n)]
    rows = S * R
    p, u = _numbers(4, rows, T, 9, dev)
    whole = _search(case, R, K, p, u, k=0.05)
    again = _search(case, R, K, p, u, k=0.05)
    _same(whole, again, "two launches")
    a = _search(case, R, K, p[:1], u[:1], k=0.05)
    b = _search(case, R, K, p[1:], u[1:], a, cycle0=1, k=0.05)
    _same(whole, b, "1 + 3", STATE)
    assert torch.equal(_bits(torch.cat([a["trace"], b["trace"]])), _bits(whole["trace"])) and torch.equal(torch.cat([a["flags"], b["flags"]]), whole["flags"])
    cur, tr, fl = None, [], []
    for c in range(4):
        cur = _search(case, R, K, p[c:c + 1], u[c:c + 1], cur, cycle0=c, k=0.05)
        tr.append(cur["trace"])
        fl.append(cur["flags"])
    _same(whole, cur, "4 x 1", STATE)
    assert torch.equal(_bits(torch.cat(tr)), _bits(whole["trace"])) and torch.equal(torch.cat(fl), whole["flags"])
    for s in range(S):
        one = _search(case, R, K, p[:, s * R:(s + 1) * R].contiguous(), u[:, s * R:(s + 1) * R].contiguous(), k=0.05, x0=case[0][s:s + 1].contiguous())
        for key in STATE:
            assert torch.equal(_bits(one[key]), _bits(whole[key][s * R:(s + 1) * R])), (s, key)
        assert torch.equal(_bits(one["trace"]), _bits(whole["trace"][:, s * R:(s + 1) * R])) and torch.equal(one["flags"], whole["flags"][:, s * R:(s + 1) * R])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole["best_e"]).all()) and int(whole["accepted"].sum()) >= 1 and int((whole["flags"] & 1).sum()) >= rows


# ---------------------------------------------------------------------------------------------- 4. forced decisions
def test_forced_metropolis_decisions_on_the_device():
    dev = _dev()
    S, R, K, n, T = 3, 3, 5, 37, 5
    case = [a.to(dev) for a in chain_case(S, n, T, 300, 91)]
    p, _ = _numbers(4, S * R, T, 3, dev)
    for value in (0.0, U_HIGH):
        u = torch.full((4, S * R), value, dtype=torch.float64, device=dev)
        st = _search(case, R, K, p, u)
        torch.cuda.synchronize()
        tr, move = st["trace"].cpu().numpy(), (st["flags"].cpu() & 1).bool().numpy()
        _, ecs, _, _, _ = replay(tr, u.cpu().numpy(), TEMP, R)
        d = tr[:, :, 1] - ecs[:-1]
        if value == 0.0:
            assert np.isfinite(tr).all() and move.all()
        else:
            clear = (d > 1e-6) | (d < 0) | ~np.isfinite(ecs[:-1])
            assert np.array_equal(move[clear], (tr[:, :, 1] < ecs[:-1])[clear]) and (~move).any() and clear.sum() >= 30
            assert np.array_equal(ecs[-1], st["best_e"][:, 3].cpu().numpy())


# ---------------------------------------------------------------------------------------------- 5. selection
def test_selection_on_crafted_energies():
    dev = _dev()
    inf, nan = float("inf"), float("nan")
    e3 = torch.tensor([1.0, -2.0, -2.0, nan, inf, 5.0, inf, inf, inf, nan, nan, nan, -1.0, -1.0, -3.0])
    be = torch.randn(15, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    be[:, 3] = e3
    pos = torch.randn(15, 37, 3, generator=torch.Generator().manual_seed(2))
    pos[3, 0, 0] = nan
    bc = torch.arange(15, dtype=torch.int32) - 1
    p, e, r, c = LA.pose_search_select(pos.to(dev), be.to(dev), bc.to(dev), 3)
    torch.cuda.synchronize()
    want = [1, 2, 0, 0, 2]
    assert r.cpu().tolist() == want == select_ref(e3.numpy(), 3).tolist()
    q = torch.tensor([3 * s + w for s, w in enumerate(want)])
    assert torch.equal(_bits(p.cpu()), _bits(pos[q])) and torch.equal(_bits(e.cpu()), _bits(be[q])) and torch.equal(c.cpu(), bc[q])
    rt = SE.select_torch(be.to(dev), pos.to(dev), bc.to(dev), 3)
    assert torch.equal(rt[2], r) and torch.equal(_bits(rt[0]), _bits(p))
    # one replica: the identity
    p1, e1, r1, c1 = LA.pose_search_select(pos.to(dev), be.to(dev), bc.to(dev), 1)
    assert torch.equal(_bits(p1.cpu()), _bits(pos)) and r1.cpu().tolist() == [0] * 15 and torch.equal(c1.cpu(), bc)
    with pytest.raises(L.DdpError):
        LA.pose_search_select(pos.to(dev), be.to(dev), bc.to(dev), 4)


# ---------------------------------------------------------------------------------------------- 6. NaN containment
def test_a_nan_sample_keeps_its_pose_by_bits_on_the_device():
    dev = _dev()
    S, R, K, n, T = 3, 2, 4, 37, 5
    case = [a.to(dev) for a in chain_case(S, n, T, 300, 17)]
    p, u = _numbers(3, S * R, T, 4, dev)
    clean = _search(case, R, K, p, u)
    bad = case[0].clone()
    bad[1, 5, 1] = float("nan")
    got = _search(case, R, K, p, u, x0=bad)
    torch.cuda.synchronize()
    for q in (2, 3):
        assert torch.equal(_bits(got["cur_pos"][q]), _bits(bad[1])) and torch.equal(_bits(got["best_pos"][q]), _bits(bad[1]))
        assert bool((got["best_e"][q] == float("inf")).all()) and bool((got["cur_e"][q] == float("inf")).all())
        assert int(got["best_cycle"][q]) == -1 and int(got["accepted"][q]) == 0 and bool((got["flags"][:, q] == 0).all())
        assert bool(torch.isnan(got["trace"][:, q]).all())
    keep = torch.tensor([0, 1, 4, 5], device=dev)
    for key in STATE:
        assert torch.equal(_bits(got[key][keep]), _bits(clean[key][keep])), key
    assert torch.equal(_bits(got["trace"][:, keep]), _bits(clean["trace"][:, keep])) and torch.equal(got["flags"][:, keep], clean["flags"][:, keep])
    _, e, r, c = LA.pose_search_select(got["best_pos"], got["best_e"], got["best_cycle"], R)
    assert int(r[1]) == 0 and int(c[1]) == -1 and float(e[1, 3]) == float("inf")


# ---------------------------------------------------------------------------------------------- 7. the 3dpf fixture
def test_the_fixture_is_never_worse_than_the_device_minimiser():
    """16 perturbed poses, R = 6, C = 4, K = 25 (96 rows): the exact inequality against PoseMinimizer(iterations=25) on the device;
    energy_after against an independent PoseScorer.score of the returned poses at the rtol of the minimiser's one-iteration test
    (1e-9); a second call with the synchronisation debug mode armed."""
    dev = _dev()
    g, _, full = fixture_3dpf()
    ps = SE.PoseSearcher(g, dev, receptor=full, config=SE.SearchConfig(replicas=6, cycles=4, iterations=25))
    x0 = perturbed_poses()
    xd = x0.to(dev)
    res = ps.search(xd)
    mres = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=25)).minimize(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x0) and res.lig_pos.is_cuda and res.trace.shape == (4, 96, 2)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res2 = ps.search(xd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(res2.lig_pos), _bits(res.lig_pos)) and torch.equal(_bits(res2.energy_after), _bits(res.energy_after))
    assert torch.equal(_bits(res.energy_minimized), _bits(mres.energy_after)) and torch.equal(_bits(res.energy_before), _bits(mres.energy_before))
    h = res.cpu()
    print("E before", [round(float(v), 2) for v in h.energy_before[:, 3]], "\nminimised", [round(float(v), 2) for v in h.energy_minimized[:, 3]],
          "\nsearched", [round(float(v), 2) for v in h.energy_after[:, 3]], "\nreplica", h.replica.tolist(), "cycle", h.cycle.tolist(),
          "moves", h.moves.tolist())
    assert bool((h.energy_after[:, 3] <= h.energy_minimized[:, 3]).all()) and bool((h.energy_minimized[:, 3] <= h.energy_before[:, 3]).all())
    sc = ps.scorer.score(res.lig_pos).cpu()

    def close(a, b):
        return bool(((a - b).abs() <= 1e-9 * b.abs() + 1e-12).all())

    assert close(h.energy_after[:, 0], sc.inter) and close(h.energy_after[:, 1], sc.intra) and close(h.energy_after[:, 3], sc.inter + sc.intra)
    assert torch.equal(h.energy_after[:, 2], torch.zeros(16, dtype=torch.float64))
    assert torch.equal(h.replica.long(), torch.as_tensor(select_ref(res.trace.cpu()[:, :, 1].min(0).values.numpy(), 6)))
    assert torch.allclose(h.rmsd_moved.double(), (h.lig_pos.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt(), atol=1e-5)


# ---------------------------------------------------------------------------------------------- 8. limits and the launch-by-launch form
def test_the_launch_by_launch_form_and_the_fall_back_above_the_limits():
    dev = _dev()
    # fused=False on a small case: the same invariants (not the same bits: the pose maps differ in their block sums)
    host = chain_case(3, 37, 5, 300, 91)
    cfg = SE.SearchConfig(replicas=2, cycles=3, iterations=5, seed=3)
    cs = chain_searcher([a.to(dev) for a in host], cfg, dev)
    x0 = host[0].to(dev)
    starts = []
    st = cs.advance(cs.start(x0), 3, fused=False, starts=starts)
    two = cs.advance(cs.advance(cs.start(x0), 1, fused=False), 2, fused=False)
    torch.cuda.synchronize()
    for key in STATE + ("trace", "flags"):
        assert torch.equal(_bits(getattr(st, key)), _bits(getattr(two, key))), key
    assert torch.equal(_bits(starts[0][::2]), _bits(x0))
    f, ecs, ebs, bc, margin = replay(st.trace.cpu().numpy(), st.u.cpu().numpy(), cfg.temperature, 2)
    assert margin > 1e-9 and np.array_equal(f, st.flags.cpu().numpy())
    assert np.array_equal(ebs[-1], st.best_e[:, 3].cpu().numpy()) and np.array_equal(bc, st.best_cycle.cpu().numpy())
    _, e, rep, _ = cs.select(st)
    assert bool((e[:, 3] <= st.energy_minimized[:, 3]).all()) and bool((st.energy_minimized[:, 3] <= st.trace[0, ::2, 0]).all())
    assert rep.cpu().tolist() == select_ref(st.best_e[:, 3].cpu().numpy(), 2).tolist()
    # replica 0 starts both device forms at the same fp32 pose: the same fp64 evaluation, up to the order of its last sums
    fused = cs.advance(cs.start(x0), 1)
    torch.cuda.synchronize()
    assert torch.allclose(fused.trace[0, ::2, 0], st.trace[0, ::2, 0], rtol=1e-12, atol=0)
    # a ligand above the limit: fused=True warns, names the limit and takes the launch-by-launch form
    copies = L.DDP_MINIMIZE_MAX_ATOMS // 37 + 1
    big_g = tiled_graph(copies)
    ps = SE.PoseSearcher(big_g, dev, config=SE.SearchConfig(replicas=2, cycles=2, iterations=2))
    assert ps.n > L.DDP_MINIMIZE_MAX_ATOMS and not ps.minimizer.fused_available()
    poses = (big_g["ligand"].pos.float()[None] + 0.2 * torch.randn(2, ps.n, 3, generator=torch.Generator().manual_seed(1))).to(dev)
    M._warned.clear()
    with pytest.warns(UserWarning, match="PoseSearcher.*DDP_MINIMIZE_MAX_ATOMS"):
        fell = ps.search(poses, fused=True)
    slow = ps.search(poses, fused=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fell.lig_pos), _bits(slow.lig_pos)) and torch.equal(_bits(fell.energy_after), _bits(slow.energy_after))
    assert bool((slow.energy_after[:, 3] <= slow.energy_minimized[:, 3]).all()) and bool((slow.energy_minimized[:, 3] <= slow.energy_before[:, 3]).all())
    # the raw entry refuses what the class does not hand it
    with pytest.raises(L.DdpError, match="DDP_MINIMIZE_MAX_ATOMS"):
        big = [poses[:1].contiguous(), torch.ones(ps.n, device=dev), torch.zeros(ps.n, dtype=torch.uint8, device=dev)] + \
              [a.to(dev) for a in host[3:6]] + [None, torch.zeros(0, 2, dtype=torch.int32, device=dev), torch.zeros(0, ps.n, dtype=torch.uint8, device=dev)]
        _search(big, 1, 1, *_numbers(1, 1, 0, 0, dev))
    with pytest.raises(L.DdpError, match="perturb"):
        case = [a.to(dev) for a in host]
        p, u = _numbers(1, 6, 5, 0, dev)
        _search(case, 2, 1, p[:, :, :7].contiguous(), u)


# ---------------------------------------------------------------------------------------------- 9. the driver on the device
def test_run_csv_searches_on_the_device(tmp_path):
    import os
    from test_gpu_trajectory import GOLDEN, _model_dir
    dev = _dev()
    model_dir = _model_dir(tmp_path, False)
    model, margs, sigma = INF._load_model(model_dir, "best_ema_inference_epoch_model.pt", dev)
    pdb, sdf = os.path.join(GOLDEN, "3dpf_protein.pdb"), os.path.join(GOLDEN, "3dpf_ligand.sdf")
    csv_path = tmp_path / "one.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                        f"3dpf,{pdb},{sdf},,,,\n")
    gk = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction", "pocket_buffer",
                                         "pocket_cutoff")}
    from diffdock_pocket_amd.sampler import SamplerConfig
    cfg = SamplerConfig(inference_steps=4, sigma=sigma, flexible_sidechains=False)
    res = INF.run_csv(str(csv_path), model, dev, samples_per_complex=3, inference_steps=4, seed=7, sampler_cfg=cfg, graph_kwargs=gk,
                      allow_zero_esm=True, out_dir=str(tmp_path / "out"), search_poses=SE.SearchConfig(replicas=3, cycles=2, iterations=3))[0]
    assert res.skipped is None, res.skipped
    sr = res.searched
    assert isinstance(sr, SE.SearchResult) and not sr.lig_pos.is_cuda and sr.lig_pos.shape == res.ligand_pos.shape
    assert torch.equal(sr.lig_pos, res.searched_pos) and sr.trace.shape == (2, 9, 2)
    assert bool((sr.energy_after[:, 3] <= sr.energy_minimized[:, 3]).all()) and bool((sr.energy_minimized[:, 3] <= sr.energy_before[:, 3]).all())
    names = {os.path.basename(f) for f in res.files}
    assert {"searched.csv", "rank1_searched.sdf", "rank2_searched.sdf", "rank3_searched.sdf"} <= names
    assert names == set(os.listdir(os.path.dirname(res.files[0])))
    torch.cuda.synchronize()
