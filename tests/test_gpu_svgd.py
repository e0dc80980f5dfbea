"""The SVGD kernels (csrc/ddp_svgd.hip: ddp_svgd_tau / ddp_svgd_pairs / ddp_svgd_rows) through the C ABI against the float64
restatement of tests/svgd_ref.py, and the device sampler with svgd_weight > 0.

Bound of the kernel-level cases: tests/golden/sampler_svgd.pt stores, for N = 5 and N = 8 poses of the 3dpf ligand, the largest
deviation `fig` of the REFERENCE's own fp32 results from the float64 restatement (relative to each output's largest magnitude); the
kernels are held to 4 fig on the same inputs (Horn's quaternion instead of an SVD, another summation order: equally valid
evaluations) and to 4 x the largest stored figure on the shapes without a golden vector.  The update buffers are one fp32 sum further:
|upd - want| <= bound * max |weight total| + 2^-24 max |upd|.

No case is left out for the three discontinuities (quaternion-candidate choice, +-pi wrap, cosine clamp): the seeds are fixed so that
the inputs keep the margins of svgd_ref.margins_ok, and every test asserts them in float64 before it compares."""
import functools
import os

import numpy as np
import pytest
import torch

import svgd_ref as R
from diffdock_pocket_amd.diffusion import SigmaRanges, get_t_schedule

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_svgd.pt")
U24 = 2.0 ** -24
LIG_DIH = np.array([[8, 7, 6, 1], [18, 17, 16, 12], [19, 18, 17, 16], [17, 18, 19, 20], [18, 19, 21, 22]], np.int32)   # 3dpf ligand


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


# name -> (N, pose source, pose seed, torsions, (w_rep, w_rot, w_tor), weight)
CASES = {
    "gold_n5": (5, "gold", None, True, (1.0, 1.0, 1.0), 0.5),            # odd median, golden inputs
    "gold_n8": (8, "gold", None, True, (1.0, 1.0, 1.0), 0.5),            # even N: the lower median, golden inputs
    "chain_n3": (3, "chain", 1, True, (0.8, 0.7, 1.3), 0.5),             # smallest N, smallest dihedral (4 atoms, T = 1)
    "chain_n65": (65, "chain", 31, True, (1.0, 1.0, 1.0), 1.5),          # a row one past a wave
    "lig_n40": (40, "lig", 23, True, (0.8, 0.7, 1.3), 0.5),              # the workload's own N, 37 atoms, T = 5, weights other than 1
    "lig_n8_t0": (8, "lig", 1, False, (1.0, 0.7, 1.0), 0.5),             # no rotatable bond
}


def _inputs(name, gold):
    N, src, seed, tors, w, weight = CASES[name]
    if src == "gold":
        pos, dih = gold["cases"][N]["lig_start"].numpy(), gold["cases"][N]["dihedrals"].numpy()
        assert np.array_equal(dih, LIG_DIH)
        bound = 4 * gold["cases"][N]["fig"]
    else:
        bound = 4 * max(c["fig"] for c in gold["cases"].values())
        pos, dih = R.chain_poses(seed, N) if src == "chain" else (R.ligand_poses(seed, N), LIG_DIH)
    dih = dih if tors else None
    T = 0 if dih is None else len(dih)
    rng = np.random.default_rng(100 + N)
    if src == "gold":      # the generator's scores: the stub score function on the start poses
        from oracle.make_golden_sampler import stub_scores
        from diffdock_pocket_amd.batch import collate
        from diffdock_pocket_amd.synthetic import make_3dpf_complex
        b = collate([make_3dpf_complex(seed=0, flexible_sidechains=False)] * N)
        b["ligand"].pos = torch.from_numpy(pos).reshape(-1, 3)
        tr, rot, tor, _ = stub_scores(b, T, 0)
        scores = [tr.numpy(), rot.numpy(), tor.reshape(N, T).numpy()]
        gdt = gold["cases"][N]["gdt"]
    else:
        scores = [rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32),
                  rng.standard_normal((N, T)).astype(np.float32) if T else None]
        gdt = R.g2dt(SigmaRanges(), 0.6, 0.05)
    base = [(0.3 * rng.standard_normal(s.shape)).astype(np.float32) if s is not None else None for s in scores]
    return pos, dih, scores, base, np.asarray(gdt, np.float32), w, weight, bound


@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_float64_restatement(gold, name, only):
    from diffdock_pocket_amd.svgd import SvgdWorkspace
    dev = _dev()
    pos, dih, scores, base, gdt, w, weight, bound = _inputs(name, gold)
    N, n_lig, T = pos.shape[0], pos.shape[1], 0 if dih is None else len(dih)
    want = R.forward(pos, dih, scores, gdt.astype(np.float64), *w)
    assert R.margins_ok(want), (name, want["q_gap"], want["wrap_gap"], want["cos_gap"])
    ws = SvgdWorkspace(N, n_lig, None if dih is None else torch.from_numpy(dih), dev, weight=weight, w_rep=w[0], w_rot=w[1], w_tor=w[2],
                       svgd_only=only)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev).contiguous()     # noqa: E731
    sc, upd = [up(s) for s in scores], [up(b) for b in base]
    ws.launch(up(pos), sc, upd, up(gdt))
    torch.cuda.synchronize()
    got = {"tr_diff": ws.tr_diff, "rot_diff": ws.rot_diff, "D": ws.dist}
    if T:
        got.update(tau=ws.tau, tor_diff=ws.tor_diff)
    for k, v in got.items():
        d = R.rel_dev(v.cpu().numpy(), want[k])
        print(f"[svgd] {name} only={only} {k}: {d:.3e} (bound {bound:.3e})")
        assert d <= bound, (name, k, d, bound)
    # the lower triangle is the negated mirror of the upper one, bit for bit; the diagonal is zero
    for v in (ws.tr_diff, ws.rot_diff):
        assert torch.equal(v, -v.transpose(0, 1)) and not bool(v[torch.arange(N), torch.arange(N)].any())
    for k in range(3 if T else 2):
        w_tot = weight * want["total"][k]
        full = R.update(base[k], want["total"][k], weight, only)
        err = float(np.abs(upd[k].cpu().numpy().astype(np.float64) - full).max())
        allowed = bound * float(np.abs(w_tot).max()) + U24 * float(np.abs(full).max())
        print(f"[svgd] {name} only={only} upd[{k}]: |err| {err:.3e} (allowed {allowed:.3e}, max |weight total| {np.abs(w_tot).max():.3e})")
        assert err <= allowed, (name, k, err, allowed)
    assert float(np.abs(want["total"][0]).max()) > 0 and np.isfinite(want["total"][0]).all()
    # a second run of the passes on the same inputs repeats the first bit for bit (no atomics, fixed summation order)
    upd2 = [up(b) for b in base]
    first = [v.clone() for v in (ws.tr_diff, ws.rot_diff, ws.dist)]
    ws.launch(up(pos), sc, upd2, up(gdt))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, (ws.tr_diff, ws.rot_diff, ws.dist)))
    assert all(torch.equal(a, b) for a, b in zip(upd[:3 if T else 2], upd2[:3 if T else 2]))


def test_abi_rejects_shapes_outside_the_definition():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd.svgd import SvgdWorkspace
    dev = _dev()
    with pytest.raises(ValueError):
        SvgdWorkspace(2, 37, None, dev)
    with pytest.raises(ValueError):
        SvgdWorkspace(5, 3, None, dev)
    with pytest.raises(ValueError):
        SvgdWorkspace(5, 4, torch.tensor([[0, 1, 2, 4]], dtype=torch.int32), dev)
    ws = SvgdWorkspace(3, 4, None, dev)
    ws.args.n = 2
    import ctypes as C
    assert L.load().ddp_svgd_pairs(C.byref(ws.args), None) == -1      # DDP_EINVAL, nothing launched


SEED = 1       # Sampler seed whose randomised start poses (no_random: torsions and rotations only) keep the margins, found on the CPU


@functools.lru_cache(maxsize=1)
def _model():
    """The small cfg1 score model with the synthetic weights of the parity cases."""
    from oracle.cases import CASES as MODEL_CASES
    from helpers import case_inputs
    from diffdock_pocket_amd.score_model import TensorProductScoreModel
    case = MODEL_CASES["cfg1_full"]
    kw = dict(case.model_kwargs())
    kw.update(case.ctor_extras())
    kw["device"] = _dev()
    model = TensorProductScoreModel(**kw)
    model.load_state_dict(case_inputs(case.name)[3], strict=True)
    return model.to(_dev()).eval()


def _sampler(only=False, graph=False, n=5, sl=None, steps=20):
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    model = _model()
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=16)
    cfg = SamplerConfig(inference_steps=steps, flexible_sidechains=False, no_random=True, hip_graph=graph, svgd_weight=0.5, svgd_only=only,
                        svgd_rot_rel_weight=0.7, svgd_tor_rel_weight=1.3, svgd_repulsive_weight=0.8)
    return Sampler(model, g, n, _dev(), cfg, seed=SEED, sample_slice=sl), g


@pytest.mark.parametrize("only", [False, True])
def test_one_device_step_matches_the_restatement(only):
    """One uncaptured step = the float64 restatement applied to scores(t) and the pre-step poses, then the PyTorch modify_conformer:
    2e-4 A, the tolerance of the project's end-to-end sampler tests."""
    from diffdock_pocket_amd import sampler as S
    smp, g = _sampler(only=only)
    smp.randomize()
    sched = get_t_schedule(20)
    pos0 = smp.lig_pos.clone().cpu()
    tr, rot, tor = [s.clone().float().cpu() for s in smp.scores(float(sched[0]))[:3]]
    smp.step(0, sched)
    torch.cuda.synchronize()
    T = smp.T
    dih = smp.svgd_dih.numpy()
    cfg = smp.cfg
    want = R.forward(pos0.numpy(), dih, [tr.numpy(), rot.numpy(), tor.reshape(5, T).numpy()], smp._svgd_gdt(0, sched),
                     cfg.svgd_repulsive_weight, cfg.svgd_rot_rel_weight, cfg.svgd_tor_rel_weight)
    assert R.margins_ok(want), (want["q_gap"], want["wrap_gap"], want["cos_gap"])
    _, coef, _ = smp._step_coefficients(0, sched)
    base = [coef[0] * tr.numpy().astype(np.float64), coef[2] * rot.numpy().astype(np.float64),
            coef[4] * tor.reshape(5, T).numpy().astype(np.float64)]
    upd = [torch.from_numpy(R.update(base[k], want["total"][k], cfg.svgd_weight, only)).float() for k in range(3)]
    for k, name in enumerate(("tr", "rot", "tor")):
        assert R.rel_dev(smp.upd[name].cpu().numpy(), upd[k].numpy()) < 1e-5, name      # (the step did use these updates)
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2], smp.bonds, [i.cpu() for i in smp.rot_idx])
    d = float((smp.lig_pos.cpu() - expect).abs().max())
    print(f"[svgd] device step only={only}: poses differ by {d:.3e} A; moved {float((expect - pos0).abs().max()):.3f} A")
    assert d < 2e-4
    assert float(np.abs(cfg.svgd_weight * want["total"][0]).max()) > 1e-3       # the term did contribute


def test_graph_replay_equals_launch_by_launch_bitwise():
    sched = get_t_schedule(20)
    out = []
    for graph in (False, True):
        smp, _ = _sampler(graph=graph)
        smp.randomize()
        for i in range(5):
            smp.step(i, sched)
        torch.cuda.synchronize()
        assert bool(smp._graph) == graph
        out.append(smp.lig_pos.clone())
        smp.close()
    assert torch.isfinite(out[0]).all() and torch.equal(out[0], out[1])


def test_sliced_sampler_raises_on_the_device():
    with pytest.raises(ValueError, match="one device"):
        _sampler(n=6, sl=slice(0, 3))
