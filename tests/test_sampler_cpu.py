"""CPU tests of the caller side: batched pose update vs golden vectors produced by the reference's own
utils/diffusion_utils.py / utils/torsion.py / utils/geometry.py, perturbation formulas, and shard invariance of the
sample-sharded sampler over a 2-rank gloo group (stub score function - the real model is HIP only)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.synthetic import make_3dpf_complex

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_pose_update.pt")


def test_pose_update_matches_reference_functions():
    g = torch.load(GOLD, weights_only=False)
    base = make_3dpf_complex(seed=0, flexible_sidechains=True)
    n = g["tr"].shape[0]
    em = base["ligand"].edge_mask
    bonds = base["ligand", "ligand"].edge_index.t()[em]
    mr = torch.as_tensor(base["ligand"].mask_rotate)
    fr = base["flexResidues"]
    atom0 = base["atom"].pos.unsqueeze(0).repeat(n, 1, 1)
    atom = S.apply_sidechain_torsions(atom0, fr.edge_idx, fr.subcomponents, fr.subcomponentsMapping, g["sc"])
    lig = S.modify_conformer(g["lig_start"], g["tr"], g["rot"], g["tor"], bonds, mr)
    assert float((S.rotvec_to_matrix(g["rot"]) - g["rot_mat"]).abs().max()) < 1e-6
    assert float((atom - g["atom_out"]).abs().max()) < 2e-4       # reference goes through float64 numpy/scipy
    assert float((lig - g["lig_out"]).abs().max()) < 2e-4


def test_kabsch_recovers_rigid_motion():
    torch.manual_seed(0)
    A = torch.randn(5, 20, 3)
    R = S.rotvec_to_matrix(torch.randn(5, 3))
    t = torch.randn(5, 1, 3)
    B = A @ R.transpose(1, 2) + t
    Rk, tk = S.kabsch(A, B)
    assert torch.allclose(Rk, R, atol=1e-5) and torch.allclose(tk, t, atol=1e-4)


class StubModel:
    """Deterministic stand-in for the score model (pure function of the batch), CPU only, for sharding tests."""

    def __init__(self, T, S_):
        self.T, self.S = T, S_

    def __call__(self, b):
        B = b.num_graphs
        lp = b["ligand"].pos.reshape(B, -1, 3)
        ap = b["atom"].pos.reshape(B, -1, 3)
        c = lp.mean(1)
        tr = -0.05 * c
        rot = 0.02 * torch.stack([c[:, 1], -c[:, 0], c[:, 2]], 1)
        tor = 0.01 * lp[:, :self.T, 0].reshape(-1)
        sc = 0.01 * ap[:, :self.S, 1].reshape(-1)
        return tr, rot, tor, sc


def _restated_plan(cfg, t_idx, sched):
    """(g2dt [4], coef [8], noise off) of a step: an fp64 restatement of reference utils/sampling.py - :94-98 (dt, the last step's dt = t),
    utils/diffusion_utils.py t_to_sigma (sigma = min^(1 - t) max^t), :129-163 (g of each component, the SDE and the ODE half), :177-195
    (lambda and psi of low-temperature sampling), :136 (when the noise is zero) - for k = tr, rot, tor, side chains."""
    sg, steps = cfg.sigma, len(sched)
    t = np.float64(sched[t_idx])
    dt = np.float64(sched[t_idx] - sched[t_idx + 1]) if t_idx < steps - 1 else t
    ranges = ((sg.tr_sigma_min, sg.tr_sigma_max), (sg.rot_sigma_min, sg.rot_sigma_max), (sg.tor_sigma_min, sg.tor_sigma_max),
              (sg.sidechain_tor_sigma_min, sg.sidechain_tor_sigma_max))
    g2dt, coef = [], []
    for k, (lo, hi) in enumerate(ranges):
        sigma = np.float64(lo) ** (1 - t) * np.float64(hi) ** t
        g = 2 * sigma * np.sqrt(np.log(hi / lo)) if k == 1 else sigma * np.sqrt(2 * np.log(hi / lo))
        temp, psi = cfg.temp_sampling[k], cfg.temp_psi[k]
        if cfg.ode:
            a, b = 0.5 * g ** 2 * dt, 0.0
        elif temp != 1.0:
            sigma_data = np.exp(cfg.temp_sigma_data * np.log(hi) + (1 - cfg.temp_sigma_data) * np.log(lo))
            lam = (sigma_data + sigma) / (sigma_data + sigma / temp)
            a, b = g ** 2 * dt * (lam + temp * psi / 2), g * np.sqrt(dt * (1 + psi))
        else:
            a, b = g ** 2 * dt, g * np.sqrt(dt)
        g2dt.append(g ** 2 * dt)
        coef += [a, b]
    return np.array(g2dt), np.array(coef), bool(cfg.no_random or (cfg.no_final_step_noise and t_idx == steps - 1))


@pytest.mark.parametrize("fields", [{}, dict(ode=True), dict(temp_sampling=(1.0, 1.0, 1.0, 1.0)), dict(no_final_step_noise=True), dict(no_random=True)],
                         ids=["default", "ode", "temp_sampling_1", "no_final_step_noise", "no_random"])
def test_step_plan_matches_the_restated_formulas(fields):
    """step_plan - the one place of sigma, g, lambda, dt and the last-step rule - against the restatement above at every step of the
    20-step schedule: 1e-14 relative (two fp64 evaluations that associate differently differ by a few ulp of 1.1e-16, no more)."""
    cfg = S.SamplerConfig(inference_steps=20, **fields)
    sched = get_t_schedule(20)
    smp = S.Sampler(StubModel(0, 0), make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20), 2, torch.device("cpu"), cfg)
    for t_idx in range(20):
        plan = S.step_plan(cfg, t_idx, sched)
        g2dt, coef, noise_off = _restated_plan(cfg, t_idx, sched)
        assert plan.t == float(sched[t_idx]) and plan.dt == (plan.t if t_idx == 19 else float(sched[t_idx] - sched[t_idx + 1]))
        assert len(plan.g2dt) == 4 and len(plan.coef) == 8
        np.testing.assert_allclose(np.array(plan.g2dt), g2dt, rtol=1e-14, atol=0)
        np.testing.assert_allclose(np.array(plan.coef), coef, rtol=1e-14, atol=0)
        assert plan.noise_off is noise_off
        assert noise_off == ("no_random" in fields or ("no_final_step_noise" in fields and t_idx == 19))
        assert (plan.w_clash, plan.w_score) == (0.0, 0.0)
        assert smp._step_coefficients(t_idx, sched) == (plan.t, list(plan.coef), plan.noise_off)


T_MAX = 0.6          # between the points 0.75 and 0.5 of the 4-step schedule
GUIDED = dict(clash_guidance_weight=0.5, clash_guidance_t_max=T_MAX, score_guidance_weight=0.3, score_guidance_t_max=T_MAX,
              score_guidance_sidechains=True)
STREAM_CASES = {     # name -> (SamplerConfig fields, sample_slice of 4 samples, step)
    "flexible_recorded": (dict(record_trajectory=True), None, 0),
    "rigid_svgd": (dict(flexible_sidechains=False, svgd_weight=0.5), None, 1),
    "no_torsion": (dict(no_torsion=True), None, 0),
    "slice_1_3": ({}, slice(1, 3), 2),
    "last_step_no_final_noise": (dict(no_final_step_noise=True), None, 3),
    "guided_above_t_max": (GUIDED, None, 1),
    "guided_below_t_max": (GUIDED, None, 2),
}


@pytest.mark.parametrize("case", list(STREAM_CASES))
def test_cpu_step_and_device_row_consume_the_same_noise_stream(case):
    """The CPU step (sampler A) and the host row of the device step's parameter block (sampler B: _draw_noise -> _fill_step_row, no
    device needed) leave the seeded generator in the same state, and the row holds - bit for bit - the draws of the reference loop's order
    tr, rot, tor, side chains for all 4 samples, sliced to the shard (drawn here from the generator of a third sampler), behind the time,
    the trajectory slot, SVGD's g^2 dt, the guidance weights and the SDE coefficients."""
    fields, sl, t_idx = STREAM_CASES[case]
    steps, N = 4, 4
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20)
    T, S_ = int(g["ligand"].edge_mask.sum()), int(g["flexResidues"].edge_idx.shape[0])
    cfg = S.SamplerConfig(inference_steps=steps, **fields)
    sched = get_t_schedule(steps)
    A, B, C = (S.Sampler(StubModel(T, S_), g, N, torch.device("cpu"), cfg, seed=5, sample_slice=sl) for _ in range(3))
    for smp in (A, B, C):
        smp.randomize()
    start = C.gen.get_state()
    A.step(t_idx, sched)
    plan = S.step_plan(cfg, t_idx, sched)
    n = B.n
    T_row, S_row = (0 if cfg.no_torsion else T), (S_ if cfg.flexible_sidechains else 0)
    assert B._n_par == 16 + n * (6 + T_row + S_row)
    row = torch.full((B._n_par,), float("nan"))                 # every word has to be written
    B._fill_step_row(row, plan, B._draw_noise(plan.noise_off), t_idx)
    assert torch.equal(A.gen.get_state(), B.gen.get_state())
    # the noise: the same seed's stream, drawn for all N samples in the order tr, rot, tor, side chains
    o = 16
    for cols in (3, 3, T_row, S_row):
        if cols:
            want = torch.zeros(N, cols) if plan.noise_off else torch.randn((N, cols), generator=C.gen)
            assert torch.equal(row[o:o + n * cols], want[sl or slice(0, N)].reshape(-1)), (case, o)
            o += n * cols
    assert o == B._n_par
    assert torch.equal(C.gen.get_state(), B.gen.get_state())
    assert torch.equal(B.gen.get_state(), start) == plan.noise_off      # zeros draw nothing, noise moves the stream
    before = C.gen.get_state()
    torch.randn((N, 0), generator=C.gen)                        # an empty draw (a complex without torsions of a kind) takes nothing
    assert torch.equal(C.gen.get_state(), before)
    # the slots in front of the noise
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
    t = float(sched[t_idx])
    assert row[0] == f32(t) and row[7] == 0
    assert row[1] == (t_idx + 1 if cfg.record_trajectory else 0)
    assert torch.equal(row[2:5], f32(plan.g2dt[:3]) if cfg.svgd_weight > 0 else torch.zeros(3))
    assert row[5] == f32(cfg.clash_guidance_weight if t <= cfg.clash_guidance_t_max else 0.0)
    assert row[6] == f32(cfg.score_guidance_weight if t <= cfg.score_guidance_t_max else 0.0)
    assert bool(row[5] > 0) == bool(row[6] > 0) == (case == "guided_below_t_max")
    assert torch.equal(row[8:16], f32(plan.coef))


def _run(n_total, sl, seed=3, steps=4):
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20)
    T, S_ = int(g["ligand"].edge_mask.sum()), int(g["flexResidues"].edge_idx.shape[0])
    cfg = S.SamplerConfig(inference_steps=steps)
    smp = S.Sampler(StubModel(T, S_), g, n_total, torch.device("cpu"), cfg, seed=seed, sample_slice=sl)
    smp.randomize()
    return smp.run(get_t_schedule(steps))


def _worker(rank, world, n_total, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = n_total // world
    lig, atom = _run(n_total, slice(rank * per, (rank + 1) * per))
    out = [torch.empty_like(lig) for _ in range(world)]
    dist.all_gather(out, lig.contiguous())
    if rank == 0:
        q.put(torch.cat(out, 0))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_is_shard_invariant():
    """Samples are sharded over ranks (no data-path collective), noise is drawn for the whole job and sliced; the
    gathered poses equal a single-process run bit for bit."""
    n_total = 6
    full, _ = _run(n_total, slice(0, n_total))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    import socket
    with socket.socket() as sk:          # a port that is free right now (a fixed one may still be in TIME_WAIT)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, n_total, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    gathered = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert gathered.shape == full.shape
    assert torch.equal(gathered, full)


def test_sampler_steps_match_the_reference_loop():
    """Sampler.step (scores -> SDE perturbation with the low-temperature branch -> side-chain and ligand pose update) against
    the reference's OWN loop utils/sampling.py:93-251, run unmodified for three steps on three poses with a stub score function
    of the positions and a seeded global RNG (tests/golden/sampler_loop.pt, oracle/make_golden_sampler.py).  The same seed on
    the Sampler's generator gives the same normal draws in the same order (tr, rot, tor, side chains), so the trajectories
    agree to the fp32 rounding of the pose update (the reference rotates in float64 numpy / scipy)."""
    from oracle.make_golden_sampler import LOOP_N, loop_inputs, stub_scores
    gold = torch.load(os.path.join(os.path.dirname(GOLD), "sampler_loop.pt"), weights_only=True)
    base, graphs = loop_inputs()
    assert torch.equal(torch.stack([d["ligand"].pos for d in graphs]), gold["lig_start"])
    T, S_ = int(base["ligand"].edge_mask.sum()), int(base["flexResidues"].edge_idx.shape[0])
    steps = gold["steps"]
    smp = S.Sampler(lambda b: stub_scores(b, T, S_), base, LOOP_N, torch.device("cpu"), S.SamplerConfig(inference_steps=steps),
                    seed=gold["seed"])
    smp.lig_pos, smp.atom_pos = gold["lig_start"].clone(), gold["atom_start"].clone()
    sched = get_t_schedule(steps)
    for i in range(steps):
        assert float((smp.lig_pos - gold["lig_traj"][i]).abs().max()) < 5e-4, i      # poses at the start of step i
        smp.step(i, sched)
    assert float((smp.lig_pos - gold["lig_out"]).abs().max()) < 5e-4
    assert float((smp.atom_pos - gold["atom_out"]).abs().max()) < 5e-4
    assert float((gold["lig_out"] - gold["lig_start"]).abs().max()) > 1.0            # the ligands moved by angstroms
    assert float((gold["atom_out"] - gold["atom_start"]).abs().max()) > 0.1          # and side chains turned
