"""Golden vectors for the SVGD particle-interaction term, produced by the reference's OWN functions imported under oracle/shim.py
(fixture-generation time only: needs the reference checkout):
  utils/torsion.py:96-113     get_dihedrals
  utils/torsion.py:138-145    get_torsion_angles_svgd      (tau through get_torsion_angles, :120-135)
  utils/torsion.py:148-160    get_rigid_svgd               (one SVD + matrix_to_axis_angle per pair)
  utils/sampling.py:70-251    sampling(svgd_weight=0.5)    three steps, with and without svgd_only
on N = 5 and N = 8 randomised poses of the 3dpf ligand (37 atoms, 5 rotatable bonds, rigid receptor) with the stub score function and
the loader stand-in of oracle/make_golden_sampler.py, the global RNG seeded as for tests/golden/sampler_loop.pt.  N = 3 is left out:
the reference's `torch.cross` without `dim` picks the first axis of size 3 there.

The update totals are not returned by sampling(): a wrapper around the modify_conformer it calls records the (tr, rot, tor) updates of
the first step of the svgd_only run, which are svgd_weight * total_X.

For every case the largest deviation of the reference's fp32 results from the float64 restatement (tests/svgd_ref.py), relative to each
output's largest magnitude, is stored (`dev`: per output; `fig`: their maximum - the yardstick of tests/test_gpu_svgd.py) and printed into
profiles/svgd_parity.txt.
Usage: python -m tools.make_golden_svgd
"""
import argparse
import copy
import functools
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svgd_ref as R                                                              # noqa: E402
from diffdock_pocket_amd.batch import collate                                     # noqa: E402
from diffdock_pocket_amd.diffusion import SigmaRanges                             # noqa: E402
from diffdock_pocket_amd.sampler import TEMP_PSI, TEMP_SAMPLING, TEMP_SIGMA_DATA  # noqa: E402
from diffdock_pocket_amd.synthetic import make_3dpf_complex                       # noqa: E402
from oracle import shim                                                           # noqa: E402
from oracle.make_golden_sampler import LOOP_SEED, LOOP_STEPS, stub_scores         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampler_svgd.pt")
REPORT = os.path.join(ROOT, "profiles", "svgd_parity.txt")
POSE_SEEDS = {5: 1, 8: 1}      # first seeds of svgd_ref.ligand_poses at which the margins of svgd_ref.margins_ok hold (checked below)
WEIGHT = 0.5


def main():
    ref = shim.import_reference()

    class Loader:   # stand-in for torch_geometric.loader.DataLoader, as in oracle/make_golden_sampler.py
        def __init__(self, data_list, batch_size=32):
            self.data_list, self.bs = data_list, batch_size

        def __iter__(self):
            for i in range(0, len(self.data_list), self.bs):
                yield collate(self.data_list[i:i + self.bs])

    sys.modules["torch_geometric.loader"].DataLoader = Loader
    sampling_mod = importlib.import_module("utils.sampling")
    sampling_mod.DataLoader = Loader
    base = make_3dpf_complex(seed=0, flexible_sidechains=False)
    T = int(base["ligand"].edge_mask.sum())
    sg = SigmaRanges()
    margs = argparse.Namespace(tr_sigma_min=sg.tr_sigma_min, tr_sigma_max=sg.tr_sigma_max, rot_sigma_min=sg.rot_sigma_min,
                               rot_sigma_max=sg.rot_sigma_max, tor_sigma_min=sg.tor_sigma_min, tor_sigma_max=sg.tor_sigma_max,
                               sidechain_tor_sigma_min=sg.sidechain_tor_sigma_min, sidechain_tor_sigma_max=sg.sidechain_tor_sigma_max,
                               no_torsion=False, flexible_sidechains=False, all_atoms=True)
    t_to_sigma = functools.partial(ref.diffusion_utils.t_to_sigma, args=margs)
    sched = np.linspace(1, 0, LOOP_STEPS + 1)[:-1]
    res, lines = {"seed": LOOP_SEED, "steps": LOOP_STEPS, "weight": WEIGHT, "cases": {}}, []
    for N, pose_seed in POSE_SEEDS.items():
        start = torch.from_numpy(R.ligand_poses(pose_seed, N))

        def graphs():
            out = []
            for i in range(N):
                d = copy.deepcopy(base)
                d["ligand"].pos = start[i].clone()
                out.append(d)
            return out

        data = graphs()
        dih = ref.torsion.get_dihedrals(data)
        tor_mat, tor_d = ref.torsion.get_torsion_angles_svgd(dih, start)
        tau = ref.torsion.get_torsion_angles(dih, start)
        tr_mat, rot_mat, tr_d, rot_d = ref.torsion.get_rigid_svgd(start)
        case = {"lig_start": start, "dihedrals": dih.to(torch.int32), "tau": tau, "tor_diff": tor_d, "tr_diff": tr_d, "rot_diff": rot_d}

        recorded = []
        real_mc = sampling_mod.modify_conformer

        def spy(data, tr_update, rot_update, torsion_updates, **kw):
            recorded.append((tr_update.clone().reshape(3), rot_update.clone().reshape(3), torch.as_tensor(np.array(torsion_updates))))
            return real_mc(data, tr_update, rot_update, torsion_updates, **kw)

        for only in (False, True):
            recorded.clear()
            sampling_mod.modify_conformer = spy
            torch.manual_seed(LOOP_SEED)
            try:
                out, _ = sampling_mod.sampling(
                    graphs(), lambda b: stub_scores(b, T, 0), LOOP_STEPS, sched, sched, sched, sched, torch.device("cpu"), t_to_sigma,
                    margs, batch_size=3, temp_sampling=list(TEMP_SAMPLING), temp_psi=list(TEMP_PSI), temp_sigma_data=TEMP_SIGMA_DATA,
                    return_full_trajectory=False, svgd_weight=WEIGHT, svgd_only=only)
            finally:
                sampling_mod.modify_conformer = real_mc
            case["lig_out_only" if only else "lig_out"] = torch.stack([d["ligand"].pos.float() for d in out])
        first = recorded[:N]       # (svgd_only run) the first step's updates = WEIGHT * total_X
        case["upd_only"] = [torch.stack([f[k].float() for f in first]) for k in range(3)]

        # the reference's own fp32 error against the float64 restatement, on these inputs
        scores = [s.numpy() for s in stub_scores(collate(data), T, 0)[:3]]
        scores[2] = scores[2].reshape(N, T)
        gdt = R.g2dt(sg, float(sched[0]), float(sched[0] - sched[1]))
        want = R.forward(start.numpy(), dih.numpy(), scores, gdt)
        assert R.margins_ok(want), (N, pose_seed, want["q_gap"], want["wrap_gap"], want["cos_gap"])
        dev = {"tau": R.rel_dev(tau.numpy(), want["tau"]), "tr_diff": R.rel_dev(tr_d.numpy(), want["tr_diff"]),
               "rot_diff": R.rel_dev(rot_d.numpy(), want["rot_diff"]), "tor_diff": R.rel_dev(tor_d.numpy(), want["tor_diff"])}
        for k, name in enumerate(("tr", "rot", "tor")):
            dev["upd_" + name] = R.rel_dev(case["upd_only"][k].numpy(), WEIGHT * want["total"][k])
        case["dev"] = dev
        case["fig"] = max(v for k, v in dev.items() if k != "tau")
        case["gdt"] = gdt
        res["cases"][N] = case
        lines.append(f"N = {N} (pose seed {pose_seed}): margins q_abs gap {want['q_gap']:.3e}, pi - max|tor_diff| {want['wrap_gap']:.3e}, "
                     f"1 - max|cos| {want['cos_gap']:.3e}; |rot_diff| > pi in "
                     f"{int((np.linalg.norm(want['rot_diff'], axis=-1) > np.pi).sum())} of {N * (N - 1)} entries")
        lines.append("  reference fp32 vs float64 restatement, max |d| / max |ref|: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items())
                     + f"  -> figure {case['fig']:.3e}")
        lines.append(f"  ligand moved by up to {float((case['lig_out'] - start).norm(dim=-1).max()):.2f} A in {LOOP_STEPS} steps "
                     f"({float((case['lig_out_only'] - start).norm(dim=-1).max()):.2f} A with svgd_only)")
    torch.save(res, OUT)
    with open(REPORT, "w") as f:
        f.write("SVGD term: the reference's own fp32 results against the float64 restatement (tools/make_golden_svgd.py)\n"
                + "\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    return lines


if __name__ == "__main__":
    main()
