"""CPU tests of the SVGD particle-interaction term (diffdock_pocket_amd/svgd.py, Sampler with svgd_weight > 0) against golden vectors
produced by the reference's own get_dihedrals / get_torsion_angles_svgd / get_rigid_svgd / sampling() (tests/golden/sampler_svgd.pt,
tools/make_golden_svgd.py) and against the float64 restatement of tests/svgd_ref.py.

Tolerances: the golden file stores, per case, the largest deviation `fig` of the reference's own fp32 results from the float64
restatement, relative to each output's largest magnitude.  The package's fp32 PyTorch form is another fp32 evaluation of the same
definition and is held to 4 fig against float64 (the bound the kernels get in tests/test_gpu_svgd.py), hence to 5 fig against the golden
vectors themselves."""
import math
import os

import numpy as np
import pytest
import torch

import svgd_ref as R
from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd import svgd
from diffdock_pocket_amd.diffusion import SigmaRanges, get_t_schedule
from diffdock_pocket_amd.synthetic import make_3dpf_complex

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_svgd.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


@pytest.fixture(scope="module")
def base():
    return make_3dpf_complex(seed=0, flexible_sidechains=False)


def _stub(T):
    from oracle.make_golden_sampler import stub_scores
    return lambda b: stub_scores(b, T, 0)


def _scores(base, pos):
    """The stub score function on poses pos [N, n, 3]: (tr, rot, tor [N, T]) float32."""
    from diffdock_pocket_amd.batch import collate
    N, T = pos.shape[0], int(base["ligand"].edge_mask.sum())
    b = collate([base] * N)
    b["ligand"].pos = pos.reshape(-1, 3)
    tr, rot, tor, _ = _stub(T)(b)
    return tr, rot, tor.reshape(N, T)


def test_dihedral_table_equals_the_reference(gold, base):
    dih = svgd.dihedrals(base["ligand", "ligand"].edge_index, base["ligand"].edge_mask)
    assert dih.dtype == torch.int32 and dih.shape == (5, 4)
    for N, case in gold["cases"].items():
        assert torch.equal(dih, case["dihedrals"]), N
    # (a, b) are the masked edge_index columns, in order
    em = base["ligand"].edge_mask.bool()
    assert torch.equal(dih[:, 1:3].long(), base["ligand", "ligand"].edge_index.t()[em])


@pytest.mark.parametrize("N", [5, 8])
def test_float64_restatement_reproduces_the_stored_figures(gold, base, N):
    """The yardstick itself: the restatement against the reference's fp32 outputs gives the deviations the generator stored, and the
    inputs keep their distance from the three discontinuities."""
    case = gold["cases"][N]
    pos = case["lig_start"]
    want = R.forward(pos.numpy(), case["dihedrals"].numpy(), [s.numpy() for s in _scores(base, pos)], case["gdt"])
    assert R.margins_ok(want), (want["q_gap"], want["wrap_gap"], want["cos_gap"])
    assert int((np.linalg.norm(want["rot_diff"], axis=-1) > math.pi).sum()) > 0        # the unstandardised quaternion sign shows
    for k in ("tr_diff", "rot_diff", "tor_diff"):
        assert R.rel_dev(case[k].numpy(), want[k]) == pytest.approx(case["dev"][k], rel=1e-6), k
    for k, name in enumerate(("tr", "rot", "tor")):
        assert R.rel_dev(case["upd_only"][k].numpy(), gold["weight"] * want["total"][k]) == pytest.approx(case["dev"]["upd_" + name], rel=1e-6)
    assert case["fig"] == max(v for k, v in case["dev"].items() if k != "tau") and case["fig"] < 1e-5


@pytest.mark.parametrize("N", [5, 8])
def test_pytorch_form_matches_golden_and_float64(gold, base, N):
    case = gold["cases"][N]
    pos, dih, fig = case["lig_start"], case["dihedrals"], case["fig"]
    sc = _scores(base, pos)
    want = R.forward(pos.numpy(), dih.numpy(), [s.numpy() for s in sc], case["gdt"])
    tau = svgd.torsion_angles(dih, pos)
    tr_d, rot_d = svgd.rigid_diffs(pos)
    got = {"tau": tau, "tor_diff": svgd.torsion_diffs(tau), "tr_diff": tr_d, "rot_diff": rot_d}
    for k, v in got.items():
        d64, dg = R.rel_dev(v.numpy(), want[k]), R.rel_dev(v.numpy(), case[k].numpy().reshape(v.shape))
        print(f"[svgd] N={N} {k}: vs float64 {d64:.3e}, vs golden {dg:.3e} (fig {fig:.3e})")
        assert d64 <= 4 * fig and dg <= 5 * fig, (k, d64, dg, fig)
    assert torch.equal(rot_d, -rot_d.transpose(0, 1)) and torch.equal(tr_d, -tr_d.transpose(0, 1))      # negated mirror, zero diagonal
    tot = svgd.totals(pos, dih, *sc, case["gdt"])
    for k, name in enumerate(("tr", "rot", "tor")):
        d64 = R.rel_dev(tot[k].numpy(), want["total"][k])
        dg = R.rel_dev(gold["weight"] * tot[k].numpy(), case["upd_only"][k].numpy())
        print(f"[svgd] N={N} total_{name}: vs float64 {d64:.3e}, vs golden {dg:.3e} (fig {fig:.3e})")
        assert d64 <= 4 * fig and dg <= 5 * fig, (name, d64, dg, fig)


def test_relative_weights_lower_median_and_no_torsions(gold, base):
    """Weights other than 1, an even N (lower median) and T = 0 through the PyTorch form against float64 (no golden vector: 4 x the
    largest stored figure)."""
    bound = 4 * max(c["fig"] for c in gold["cases"].values())
    pos = torch.from_numpy(R.ligand_poses(1, 8))
    dih = svgd.dihedrals(base["ligand", "ligand"].edge_index, base["ligand"].edge_mask)
    sc = _scores(base, pos)
    gdt = R.g2dt(SigmaRanges(), 0.5, 0.05)
    for d, s3 in ((dih, sc[2]), (None, None)):
        want = R.forward(pos.numpy(), None if d is None else d.numpy(), [sc[0].numpy(), sc[1].numpy(), None if s3 is None else s3.numpy()],
                         gdt, 0.8, 0.7, 1.3)
        med = np.sort(want["D"], 1)[:, 3]
        assert np.array_equal(med, torch.median(torch.from_numpy(want["D"]), dim=1)[0].numpy())      # rank 3 of 8: the lower middle value
        tot = svgd.totals(pos, d, sc[0], sc[1], s3, gdt, 0.8, 0.7, 1.3)
        assert (tot[2] is None) == (d is None)
        for k in range(3 if d is not None else 2):
            assert R.rel_dev(tot[k].numpy(), want["total"][k]) <= bound, k


@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("N", [5, 8])
def test_cpu_sampler_matches_the_reference_loop(gold, base, N, only):
    """Sampler.step with svgd_weight = 0.5 against the reference's own sampling() over three steps: same seeded noise stream, the
    poses agree to the fp32 rounding of the pose update (the reference rotates in float64 numpy / scipy; 5e-4 A as in
    tests/test_sampler_cpu.py::test_sampler_steps_match_the_reference_loop)."""
    case = gold["cases"][N]
    T, steps = int(base["ligand"].edge_mask.sum()), gold["steps"]
    cfg = S.SamplerConfig(inference_steps=steps, flexible_sidechains=False, svgd_weight=gold["weight"], svgd_only=only)
    smp = S.Sampler(_stub(T), base, N, torch.device("cpu"), cfg, seed=gold["seed"])
    smp.lig_pos = case["lig_start"].clone()
    sched = get_t_schedule(steps)
    for i in range(steps):
        smp.step(i, sched)
    want = case["lig_out_only" if only else "lig_out"]
    d = float((smp.lig_pos - want).abs().max())
    print(f"[svgd] N={N} svgd_only={only}: final poses differ by {d:.3e} A")
    assert d < 5e-4
    assert float((want - case["lig_start"]).abs().max()) > 1.0
    assert float((case["lig_out_only"] - case["lig_out"]).abs().max()) > 1.0        # the two modes are different runs


def test_zero_weight_changes_nothing(base):
    T = int(base["ligand"].edge_mask.sum())
    outs = []
    for cfg in (S.SamplerConfig(inference_steps=3, flexible_sidechains=False),
                S.SamplerConfig(inference_steps=3, flexible_sidechains=False, svgd_weight=0.0, svgd_repulsive_weight=0.3, svgd_only=True,
                                svgd_rot_rel_weight=2.0, svgd_tor_rel_weight=0.5)):
        smp = S.Sampler(_stub(T), base, 4, torch.device("cpu"), cfg, seed=3)
        assert not smp.svgd and not hasattr(smp, "svgd_dih")
        smp.randomize()
        outs.append(smp.run(get_t_schedule(3))[0])
    assert torch.equal(outs[0], outs[1])
    d = S.SamplerConfig()
    assert (d.svgd_weight, d.svgd_repulsive_weight, d.svgd_only, d.svgd_rot_rel_weight, d.svgd_tor_rel_weight) == (0.0, 1.0, False, 1.0, 1.0)


def test_undefined_combinations_raise(base, tmp_path):
    T = int(base["ligand"].edge_mask.sum())
    cfg = S.SamplerConfig(inference_steps=3, flexible_sidechains=False, svgd_weight=0.5)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="at least 3 samples"):
        S.Sampler(_stub(T), base, 2, cpu, cfg)
    with pytest.raises(ValueError, match="one device"):
        S.Sampler(_stub(T), base, 6, cpu, cfg, sample_slice=slice(0, 3))
    with pytest.raises(ValueError, match="PipelinedSampler"):
        S.PipelinedSampler(_stub(T), base, 6, cpu, cfg)
    flex = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20)
    with pytest.raises(NotImplementedError, match="side chains"):
        S.Sampler(_stub(T), flex, 4, cpu, S.SamplerConfig(inference_steps=3, flexible_sidechains=True, svgd_weight=0.5))
    with pytest.raises(ValueError, match="at least 3 samples"):
        svgd.totals(torch.zeros(2, 37, 3), None, torch.zeros(2, 3), torch.zeros(2, 3), None, [1.0, 1.0, 1.0])
    from diffdock_pocket_amd.inference import run_csv
    csv_path = tmp_path / "rows.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand\n")
    with pytest.raises(ValueError, match="sharded over ranks"):
        run_csv(str(csv_path), None, cpu, samples_per_complex=6, rank=0, world=2, shard="samples", sampler_cfg=cfg)
    with pytest.raises(ValueError, match="at least 3 samples"):
        run_csv(str(csv_path), None, cpu, samples_per_complex=2, sampler_cfg=cfg)
    # a full slice is not a shard
    S.Sampler(_stub(T), base, 4, cpu, cfg, sample_slice=slice(0, 4))


def test_command_line_accepts_the_svgd_flags():
    from diffdock_pocket_amd.inference import _parser
    a = _parser().parse_args(["--svgd_weight", "0.5", "--svgd_repulsive_weight", "0.8", "--svgd_only", "--svgd_rot_rel_weight", "0.7",
                              "--svgd_tor_rel_weight", "1.3"])
    assert (a.svgd_weight, a.svgd_repulsive_weight, a.svgd_only, a.svgd_rot_rel_weight, a.svgd_tor_rel_weight) == (0.5, 0.8, True, 0.7, 1.3)
    d = _parser().parse_args([])
    assert (d.svgd_weight, d.svgd_repulsive_weight, d.svgd_only, d.svgd_rot_rel_weight, d.svgd_tor_rel_weight) == (0.0, 1.0, False, 1.0, 1.0)


def test_c_abi_declares_the_svgd_entries():
    import re
    from diffdock_pocket_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddp_hip.h")).read()
    declared = set(re.findall(r"^int\s+(ddp_svgd_[a-z]+)\s*\(", header, flags=re.M))
    assert declared == {"ddp_svgd_tau", "ddp_svgd_pairs", "ddp_svgd_rows"} and declared <= set(L.EXPORTS)
    assert "#define DDP_ABI_VERSION 17" in header
