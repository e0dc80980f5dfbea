"""The eleven constants of ddp_score_form_t reach all four kernels that take one: ddp_pose_score, ddp_pose_minimize,
ddp_pose_minimize_flex and ddp_pose_profile run at a form in which every constant differs from the default and from every other one
(tests/pose_form_cases.py, whose inputs the CPU tests check from the reference side), against the NumPy restatements at the same
constants and, where the header promises it, bit for bit against each other; and ddp_pose_score once more with the three constants
that are all 0 by default rotated among each other."""
import numpy as np
import pytest
import torch

import flexmin_ref as F
import interactions_ref as I
import pose_form_cases as P
import vinardo_ref as V
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import scoring as SC
from test_gpu_minimize_flex import Tables, device_case

pytestmark = pytest.mark.gpu
CFG = SC.ScoreConfig(**P.FORM)
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _score_inputs():
    """score_case on the device: (x, lig_r, lig_f, rec, rec_r, rec_f, pairs)."""
    if "score" not in _CACHE:
        _CACHE["score"] = [torch.from_numpy(a).to(_dev()) for a in P.score_case()[:7]]
    return _CACHE["score"]


def _score(config):
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = _score_inputs()
    e, g = LA.pose_score(x, lig_r, lig_f, rec, rec_r, rec_f, config, P.TOR_DIVISOR, pairs, with_grad=True)
    torch.cuda.synchronize()
    return e, g


def _within(e, g, ref, what):
    be, bg = V.bounds(ref)
    err, eg = np.abs(e.cpu().numpy() - ref["energy"]), np.abs(g.cpu().numpy() - ref["grad"])
    print(f"{what}: worst |err| / bound: energy {float((err / be).max()):.3e}, gradient {float((eg / bg[:, None, None]).max()):.3e}")
    return bool((err <= be).all() and (eg <= bg[:, None, None]).all())


def _minimize_state(S, width, dev):
    return (torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev),
            torch.full((S, width), -7.0, dtype=torch.float64, device=dev), torch.full((S, width), -7.0, dtype=torch.float64, device=dev))


# ---------------------------------------------------------------------------------------------- 1. every constant reaches every kernel
def test_pose_score_at_the_form():
    ref = P.score_case()[7]
    assert ref["cutoff_gap"] >= 1e-6
    e, g = _score(CFG)
    assert _within(e, g, ref, "ddp_pose_score")


def test_pose_minimize_and_minimize_flex_start_from_the_bits_of_pose_score():
    """iterations = 0, no restraint: energy_in = (inter, intra, ...) and grad of ddp_pose_minimize are ddp_pose_score's bits, and
    ddp_pose_minimize_flex without side chains, on per-sample copies of the receptor, has ddp_pose_minimize's."""
    dev = _dev()
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = _score_inputs()
    S, n, m = x.shape[0], x.shape[1], rec.shape[0]
    e, g = _score(CFG)
    step, acc, e0, e1 = _minimize_state(S, 4, dev)
    gm = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev)
    pos = x.clone()
    LA.pose_minimize(pos, x, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, None, None, step, acc, e0, e1, 0, restraint=0.0, grad=gm)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e0[:, 0:2]), _bits(e[:, 4:6])) and torch.equal(_bits(gm), _bits(g))
    assert torch.equal(_bits(e0), _bits(e1)) and torch.equal(pos, x) and int(acc.sum()) == 0
    z = np.zeros(0, np.int64)
    empty = LA.flex_tables(Tables(dict(mov=z, sc_pairs=np.zeros((0, m), np.uint8), edge=z.reshape(0, 2), mapping=z.reshape(0, 2), sub=z)), m, dev)
    recs = rec[None].repeat(S, 1, 1).contiguous()
    step, acc, f0, f1 = _minimize_state(S, 6, dev)
    gf = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev)
    LA.pose_minimize_flex(pos, x, lig_r, lig_f, recs, recs.clone(), rec_r, rec_f, CFG, pairs, None, None, empty, step, acc, f0, f1, 0, grad=gf)
    torch.cuda.synchronize()
    assert torch.equal(_bits(f0[:, [0, 1, 5]]), _bits(e0[:, [0, 1, 3]])) and torch.equal(_bits(gf), _bits(gm))
    assert torch.equal(recs, rec[None].repeat(S, 1, 1)) and torch.equal(pos, x)


def test_pose_minimize_flex_at_the_form():
    dev = _dev()
    c = P.flex_case()
    ref = c["ref"]
    assert ref["cutoff_gap"] >= 1e-6
    t = device_case(c, dev)
    S, n, n_mov = c["x"].shape[0], c["x"].shape[1], len(c["mov"])
    step, acc, e0, e1 = _minimize_state(S, 6, dev)
    gx = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev)
    gy = torch.full((S, n_mov, 3), -7.0, dtype=torch.float64, device=dev)
    x, y = t["x"].clone(), t["y"].clone()
    LA.pose_minimize_flex(x, t["x0"], t["lig_r"], t["lig_f"], y, t["y0"], t["rec_r"], t["rec_f"], CFG, t["pairs"], None, None, t["tables"], step,
                          acc, e0, e1, 0, restraint=c["k"], restraint_sc=c["k_sc"], grad=gx, grad_mov=gy)
    torch.cuda.synchronize()
    be, bgx, bgy = F.bounds(ref)
    err = np.abs(e0.cpu().numpy() - ref["energy"])
    ex, ey = np.abs(gx.cpu().numpy() - ref["grad_x"]), np.abs(gy.cpu().numpy() - ref["grad_y"])
    print(f"worst |err| / bound: energy {float((err / be).max()):.3e}, dE/dx {float((ex / bgx[:, None, None]).max()):.3e}, "
          f"dE/dy {float((ey / bgy[:, None, None]).max()):.3e}")
    assert (err <= be).all() and (ex <= bgx[:, None, None]).all() and (ey <= bgy[:, None, None]).all()
    assert torch.equal(x, t["x"]) and torch.equal(y, t["y"]) and torch.equal(_bits(e0), _bits(e1))


@pytest.mark.parametrize("n", [37, 70])
def test_pose_profile_at_the_form(n):
    """Residues of 0, 1, 12 and 65 atoms; with n = 70 the lanes past 64 read the ligand from LDS.  Bits and pair counts are exact."""
    dev = _dev()
    case = P.profile_case(n)
    ref = case[7]
    assert ref["threshold_gap"] >= 1e-6
    x, lig_r, lig_f, rec, rec_r, rec_f, ptr = (torch.from_numpy(np.asarray(a)).to(dev) for a in case[:7])
    prof, bits = LA.pose_profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr, CFG, I.CONTACT_DISTANCE)
    torch.cuda.synchronize()
    prof = prof.cpu().numpy()
    assert (prof[..., 6] == np.floor(prof[..., 6])).all()
    I.check(prof[..., :4], prof[..., 4], prof[..., 5], prof[..., 6].astype(np.int64), bits.cpu().numpy(), ref, f"ddp_pose_profile n={n}")


# ---------------------------------------------------------------------------------------------- 2. the fields the defaults cannot tell apart
def test_rotating_the_three_zero_default_fields_changes_the_score_as_the_restatement_says():
    ref, swapped = P.score_case()[7], P.score_ref_swapped()
    e, g = _score(SC.ScoreConfig(**P.SWAPPED))
    assert _within(e, g, swapped, "ddp_pose_score, rotated")
    # and that is another result: gauss, hydrophobic, hbond and inter of every sample lie outside the bound about the unrotated form
    be, _ = V.bounds(ref)
    assert (np.abs(e.cpu().numpy() - ref["energy"])[:, [0, 2, 3, 4]] > be[:, [0, 2, 3, 4]]).all()
    assert not torch.equal(_bits(e), _bits(_score(CFG)[0]))
