"""Reverse-process trajectories recorded on the device (csrc/ddp_traj.hip, ddp_traj_record, inside the captured denoising step) and
the command line end to end on the device (python -m diffdock_pocket_amd.inference --save_visualisation)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import sampler as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("flex", [False, True])
def test_recorded_slots_are_the_poses_of_every_step(flex, graph):
    """6 samples, 20 steps of the cfg2 model: slot 0 = the randomised poses, slot t + 1 = the poses read back after step t from a
    sampler that does not record (same seed); the final poses are bitwise those of that sampler, the last slot is lig_pos."""
    import bench
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    dev = _dev()
    steps = 20
    sched = get_t_schedule(steps)
    g = make_3dpf_complex(seed=0, flexible_sidechains=flex)
    model, _ = bench.build_model("cfg2", flex, dev)
    ref = S.Sampler(model, g, 6, dev, S.SamplerConfig(inference_steps=steps, flexible_sidechains=flex, hip_graph=graph), seed=3)
    ref.randomize()
    lig, atom = [ref.lig_pos.clone()], [ref.atom_pos.clone()]
    for t in range(steps):
        ref.step(t, sched)
        lig.append(ref.lig_pos.clone())
        atom.append(ref.atom_pos.clone())
    ref.check_overflow()
    assert bool(ref._graph) == graph
    ref.close()
    rec = S.Sampler(model, g, 6, dev, S.SamplerConfig(inference_steps=steps, flexible_sidechains=flex, hip_graph=graph,
                                                      record_trajectory=True), seed=3)
    rec.randomize()
    for t in range(steps):
        rec.step(t, sched)
    rec.check_overflow()
    torch.cuda.synchronize()
    assert bool(rec._graph) == graph
    assert torch.equal(rec.lig_pos, lig[-1]) and torch.equal(rec.atom_pos, atom[-1])
    assert rec.lig_traj.shape == (6, steps + 1, rec.n_l, 3)
    for k in range(steps + 1):
        assert torch.equal(rec.lig_traj[:, k], lig[k]), k
    assert torch.equal(rec.lig_traj[:, -1], rec.lig_pos)
    if flex:
        moving = rec.moving_atoms.to(dev)
        assert rec.atom_traj.shape == (6, steps + 1, moving.numel(), 3)
        for k in range(steps + 1):
            assert torch.equal(rec.atom_traj[:, k], atom[k][:, moving]), k
    else:
        assert rec.atom_traj is None
    rec.close()


def test_run_records_and_restore_rewrites_slot_zero():
    """Sampler.run (the path of run_csv) records every slot; a restore puts slot 0 back to the restored poses."""
    import bench
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    dev = _dev()
    g = make_3dpf_complex(seed=0, flexible_sidechains=True)
    model, _ = bench.build_model("cfg1", True, dev)
    smp = S.Sampler(model, g, 4, dev, S.SamplerConfig(inference_steps=5, record_trajectory=True), seed=1)
    smp.randomize()
    snap = smp.snapshot()
    smp.run()
    torch.cuda.synchronize()
    assert torch.equal(smp.lig_traj[:, 0], snap[0]) and torch.equal(smp.lig_traj[:, -1], smp.lig_pos)
    smp.lig_traj.zero_()
    smp.restore(snap)
    torch.cuda.synchronize()
    assert torch.equal(smp.lig_traj[:, 0], snap[0]) and torch.equal(smp.atom_traj[:, 0], snap[1][:, smp.moving_atoms.to(dev)])
    smp.close()


def test_out_of_range_records_are_refused_on_the_host():
    """A step index past the allocated slots and malformed buffers raise before anything is launched; a slot value outside
    [0, n_slots) in device memory writes nothing."""
    import bench
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    dev = _dev()
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    model, _ = bench.build_model("cfg1", False, dev)
    smp = S.Sampler(model, g, 2, dev, S.SamplerConfig(inference_steps=3, flexible_sidechains=False, record_trajectory=True), seed=0)
    smp.randomize()
    sched = get_t_schedule(3)
    before = smp.lig_pos.clone()
    with pytest.raises(ValueError, match="outside"):
        smp.step(3, np.concatenate([sched, sched]))
    with pytest.raises(ValueError, match="outside"):
        smp.step(-1, sched)
    torch.cuda.synchronize()
    assert torch.equal(smp.lig_pos, before)
    lig = torch.randn(2, 5, 3, device=dev)
    traj = torch.zeros(2, 4, 5, 3, device=dev)
    with pytest.raises(ValueError):
        S.record_trajectory_hip(lig, torch.zeros(2, 4, 6, 3, device=dev), torch.zeros(1, device=dev))
    with pytest.raises(ValueError):
        S.record_trajectory_hip(lig.double(), traj, torch.zeros(1, device=dev))
    with pytest.raises(ValueError):
        S.record_trajectory_hip(lig.cpu(), traj, torch.zeros(1, device=dev))
    for bad in (4.0, -1.0, float("nan")):
        S.record_trajectory_hip(lig, traj, torch.tensor([bad], device=dev))
    S.record_trajectory_hip(lig, traj, torch.tensor([2.0], device=dev))
    torch.cuda.synchronize()
    assert torch.equal(traj[:, 2], lig) and not traj[:, [0, 1, 3]].any()
    smp.close()


# ---------------------------------------------------------------------------------------------- the command line
def _model_dir(tmp_path, flex):
    """model_parameters.yml (the README score model's namespace, shrunk) + the state dict of that model."""
    import argparse
    import yaml
    from diffdock_pocket_amd import factory
    with open(os.path.join(GOLDEN, "factory_kwargs.json")) as f:
        args = dict(json.load(f)["score_README_72"]["args"])
    args.update(ns=16, nv=4, num_conv_layers=2, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                flexible_sidechains=flex, dropout=0.0)
    d = tmp_path / ("flex" if flex else "rigid")
    d.mkdir()
    with open(d / "model_parameters.yml", "w") as f:
        yaml.safe_dump(args, f)
    torch.manual_seed(0)
    m = factory.get_model(argparse.Namespace(**args), torch.device("cpu"), None, no_parallel=True)
    torch.save(m.state_dict(), d / "best_ema_inference_epoch_model.pt")
    return str(d)


@pytest.mark.parametrize("flex", [False, True])
def test_cli_end_to_end(tmp_path, flex):
    from diffdock_pocket_amd import inference as INF
    model_dir = _model_dir(tmp_path, flex)
    out = tmp_path / "out"
    pdb, sdf = os.path.join(GOLDEN, "3dpf_protein.pdb"), os.path.join(GOLDEN, "3dpf_ligand.sdf")
    argv = ["--protein_path", pdb, "--ligand", sdf, "--complex_name", "3dpf", "--model_dir", model_dir, "--out_dir", str(out),
            "--samples_per_complex", "3", "--inference_steps", "4", "--save_visualisation", "--allow_zero_esm", "--seed", "7"]
    if flex:
        argv += ["--flexible_sidechains", "A:160-A:193-A:197"]
    r = subprocess.run([sys.executable, "-m", "diffdock_pocket_amd.inference"] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = out / "index0___3dpf"
    names = set(os.listdir(d))
    want = {f"rank{k}.sdf" for k in (1, 2, 3)} | {f"rank{k}_reverseprocess.pdb" for k in (1, 2, 3)}
    if flex:
        want |= {f"rank{k}_protein.pdb" for k in (1, 2, 3)} | {f"rank{k}_reverseprocess_protein.pdb" for k in (1, 2, 3)}
    assert names == want
    # the same job in this process: the rank-1 SDF holds its first ranked pose
    dev = _dev()
    model, margs, sigma = INF._load_model(model_dir, "best_ema_inference_epoch_model.pt", dev)
    csv_path = tmp_path / "one.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                        f"3dpf,{pdb},{sdf},,,,{'A:160-A:193-A:197' if flex else ''}\n")
    gk = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction", "pocket_buffer",
                                         "pocket_cutoff")}
    if flex:
        gk["flexdist"] = float(margs.flexdist)
    cfg = S.SamplerConfig(inference_steps=4, sigma=sigma, flexible_sidechains=flex, record_trajectory=True)
    res = INF.run_csv(str(csv_path), model, dev, samples_per_complex=3, inference_steps=4, seed=7, sampler_cfg=cfg, graph_kwargs=gk,
                      allow_zero_esm=True, save_visualisation=True)[0]
    assert res.skipped is None
    oc = res.original_center.reshape(1, 3).double()
    for k in range(3):
        back = I.parse_sdf(open(d / f"rank{k + 1}.sdf").read())
        assert np.abs(back.pos - (res.ligand_pos[k].double() + oc).numpy()).max() < 1e-4
    traj = open(d / "rank1_reverseprocess.pdb").read().split("ENDMDL")[:-1]
    assert len(traj) == 4 + 1 + 2
    if flex:
        prot = I.parse_pdb(open(d / "rank1_protein.pdb").read())
        assert sum(len(r.atoms) for r in prot) > 0
        frames = open(d / "rank2_reverseprocess_protein.pdb").read().split("ENDMDL")[:-1]
        assert len(frames) == 4 + 1 + 2
