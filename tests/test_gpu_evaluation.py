"""Pose evaluation through the HIP kernels of csrc/ddp_eval.hip (ddp_pose_rmsd, ddp_pose_contacts) against the PyTorch form and
the float64 restatement of tests/test_evaluation_cpu.py: sample counts 1 / 7 / 40, 1 / 2 / 1296 permutations, atom counts near
DDP_EVAL_MAX_ATOMS, the shared and the per-sample receptor, bitwise determinism, a short device Sampler run end to end, and the
limits."""
import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import evaluation as E
from diffdock_pocket_amd import launch as LA
from test_evaluation_cpu import check_against_numpy, graph_3dpf, perturbed, tris_cf3_benzene

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_as_torch_form(got, want, lig_shape, band_ok=True):
    """HIP metrics against the PyTorch form of the same poses."""
    got = got.cpu()
    for k in ("rmsd", "rmsd_plain"):
        assert torch.allclose(getattr(got, k).double(), getattr(want, k).double(), rtol=1e-5, atol=1e-6), k
    for k in ("centroid", "min_cross", "min_self"):
        assert torch.allclose(getattr(got, k).double(), getattr(want, k).double(), rtol=0, atol=1e-5), k
    if want.sc_rmsd is not None:
        assert torch.allclose(got.sc_rmsd.double(), want.sc_rmsd.double(), rtol=1e-5, atol=1e-6)
    assert got.symmetry_corrected == want.symmetry_corrected


@pytest.mark.parametrize("S", [1, 7, 40])
@pytest.mark.parametrize("mode", ["rigid_full_receptor", "flexible_graph_receptor"])
def test_hip_matches_torch_form_and_float64(S, mode):
    dev = _dev()
    if mode == "rigid_full_receptor":
        g, pdb = graph_3dpf()
        kw = {"receptor": E.PoseEvaluator.full_receptor(pdb, g.original_center)}
    else:
        g, _ = graph_3dpf("A:160-A:193-A:197")
        kw = {}
    ev_cpu, ev = E.PoseEvaluator(g, **kw), E.PoseEvaluator(g, dev, **kw)
    lig = perturbed(g["ligand"].pos.float(), S, seed=S)
    apos = perturbed(g["atom"].pos.float(), S, scale=0.3, seed=S + 1) if mode != "rigid_full_receptor" else None
    got = ev.evaluate(lig.to(dev), None if apos is None else apos.to(dev))
    assert got.rmsd.is_cuda and got.clashes.dtype == torch.int32 and (got.sc_rmsd is None) == (apos is None)
    want = ev_cpu.evaluate(lig, apos)
    _same_as_torch_form(got, want, lig.shape)
    check_against_numpy(got, ev_cpu, lig, apos)


def test_hip_rmsd_over_many_permutations():
    """1296 permutations: five passes of the 256 lanes per sample; P = 1 through the same entry."""
    dev = _dev()
    z, ei = tris_cf3_benzene()
    perms, _ = E.ligand_automorphisms(z, ei)
    ref = torch.randn(len(z), 3, generator=torch.Generator().manual_seed(5)) * 2
    for S in (1, 7, 40):
        pred = perturbed(ref, S, scale=1.0, seed=S)
        pred[0] = ref[torch.from_numpy(perms[777]).long()]        # an exact relabelling: the minimum is 0 at p = 777
        r, b = LA.pose_rmsd(pred.to(dev), ref.to(dev), torch.from_numpy(np.ascontiguousarray(perms.T)).to(dev))
        rt, bt = E._rmsd_torch(pred, ref, torch.from_numpy(perms))
        assert torch.allclose(r.cpu().double(), rt.double(), rtol=1e-5, atol=1e-6)
        assert float(r[0]) == 0.0 and int(b[0]) == 777
        v = np.sqrt(((pred.double().numpy()[:, None] - ref.double().numpy()[perms][None]) ** 2).sum(-1).mean(-1))
        srt = np.sort(v, 1)
        clear = srt[:, 1] - srt[:, 0] > 1e-4
        assert (b.cpu().long().numpy()[clear] == bt.long().numpy()[clear]).all()
        r1, b1 = LA.pose_rmsd(pred.to(dev), ref.to(dev), torch.arange(len(z), dtype=torch.int32, device=dev)[:, None].contiguous())
        assert torch.allclose(r1.cpu().double(), torch.from_numpy(v[:, 0]), rtol=1e-5, atol=1e-6) and (b1 == 0).all()


@pytest.mark.parametrize("per_sample", [False, True])
def test_hip_near_the_atom_limit(per_sample):
    """n = DDP_EVAL_MAX_ATOMS - 3 atoms, m = 1237 receptor atoms (no multiple of 64 / 256), some receptor radii negative."""
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    n, m, S = L.DDP_EVAL_MAX_ATOMS - 3, 1237, 7
    ref = torch.randn(n, 3, generator=gen) * 6
    lig = perturbed(ref, S, scale=0.5, seed=12)
    rec = torch.randn((S, m, 3) if per_sample else (m, 3), generator=gen) * 7
    lig_r = 1.4 + 0.4 * torch.rand(n, generator=gen)
    rec_r = 1.4 + 0.4 * torch.rand(m, generator=gen)
    rec_r[::5] = -1.0
    ref_c = ref.double().mean(0).float()
    got = LA.pose_contacts(lig.to(dev), lig_r.to(dev), rec.to(dev), rec_r.to(dev), ref_c.to(dev)).cpu()
    want = E._contacts_torch(lig, lig_r, rec, rec_r, ref_c)
    assert torch.allclose(got[:, 1:], want[:, 1:], rtol=0, atol=1e-5)
    r = rec[None].expand(S, m, 3) if not per_sample else rec
    d = (lig.double()[:, :, None] - r.double()[:, None]).norm(dim=-1)
    thr = (lig_r.double()[:, None] + rec_r.double()[None] - 0.8)
    band = (((d - thr).abs() < 1e-4) & (rec_r[None, None] >= 0)).sum((1, 2))
    exact = ((d < thr) & (rec_r[None, None] >= 0)).sum((1, 2))
    assert ((got[:, 0].long() - exact).abs() <= band).all() and (got[:, 0] == got[:, 0].round()).all()
    ident = torch.arange(n, dtype=torch.int32)[:, None].contiguous()
    rr, _ = LA.pose_rmsd(lig.to(dev), ref.to(dev), ident.to(dev))
    rt, _ = E._rmsd_torch(lig, ref, ident.T)
    assert torch.allclose(rr.cpu().double(), rt.double(), rtol=1e-5)
    # the side-chain form: a row selection with the per-sample stride of a larger array
    sel = torch.arange(0, n, 3, dtype=torch.int32)
    rs, _ = LA.pose_rmsd(lig.to(dev), ref[sel.long()].contiguous().to(dev), ident[:len(sel)].contiguous().to(dev), sel=sel.to(dev))
    rst, _ = E._rmsd_torch(lig, ref[sel.long()], ident[:len(sel)].T, sel=sel.long())
    assert torch.allclose(rs.cpu().double(), rst.double(), rtol=1e-5)


def test_hip_evaluation_is_bitwise_reproducible():
    dev = _dev()
    g, _ = graph_3dpf("A:160-A:193-A:197")
    ev = E.PoseEvaluator(g, dev)
    lig = perturbed(g["ligand"].pos.float(), 40, seed=7).to(dev)
    apos = perturbed(g["atom"].pos.float(), 40, scale=0.3, seed=8).to(dev)
    a, b = ev.evaluate(lig, apos).cpu(), ev.evaluate(lig, apos).cpu()
    for k in ("rmsd", "rmsd_plain", "best_perm", "centroid", "min_cross", "min_self", "clashes", "sc_rmsd"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("flex", [False, True])
def test_device_sampler_poses_evaluate_like_the_torch_form(flex):
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from oracle.cases import CASES
    from helpers import case_inputs
    from test_gpu_parity import _model_for
    dev = _dev()
    case = CASES["cfg1_full"] if flex else CASES["cfg2_noflex"]
    _, _, _, sd = case_inputs(case.name)
    model = _model_for(case, sd)
    g = make_3dpf_complex(seed=0, flexible_sidechains=flex, n_rec=16)
    smp = Sampler(model, g, 4, dev, SamplerConfig(inference_steps=4, flexible_sidechains=flex), seed=3)
    smp.randomize()
    sched = get_t_schedule(4)
    for i in range(4):
        smp.step(i, sched)
    lig, apos = smp.lig_pos.clone(), smp.atom_pos.clone() if flex else None
    smp.close()
    ev = E.PoseEvaluator(g, dev)
    got = ev.evaluate(lig, apos)
    torch.cuda.synchronize()
    want = E.PoseEvaluator(g).evaluate(lig.cpu(), None if apos is None else apos.cpu())
    _same_as_torch_form(got, want, lig.shape)
    assert (got.sc_rmsd is not None) == flex
    check_against_numpy(got, E.PoseEvaluator(g), lig.cpu(), None if apos is None else apos.cpu())


def test_limits_and_empty_batches():
    dev = _dev()
    n = L.DDP_EVAL_MAX_ATOMS + 1
    x = torch.zeros(2, n, 3, device=dev)
    ident = torch.arange(n, dtype=torch.int32, device=dev)[:, None].contiguous()
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        LA.pose_rmsd(x, x[0].contiguous(), ident)
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        LA.pose_contacts(x, torch.ones(n, device=dev), x[0].contiguous(), torch.ones(n, device=dev), torch.zeros(3, device=dev))
    g, _ = graph_3dpf()
    ev = E.PoseEvaluator(g, dev)
    m = ev.evaluate(torch.zeros(0, ev.n, 3, device=dev))
    assert m.rmsd.shape == (0,) and m.clashes.shape == (0,) and m.rmsd.is_cuda
    torch.cuda.synchronize()
