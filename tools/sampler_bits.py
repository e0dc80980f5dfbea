"""python tools/sampler_bits.py cpu|device LABEL out.json [tensors]     python tools/sampler_bits.py check out.json
(profiles/sampler_bits.json; the device part needs an MI355X)
SHA-256 of the bytes of what a denoising step leaves behind, after every step of short seeded jobs over the sampler's configurations:
poses and generator state on the CPU (stub score model of tests/test_sampler_cpu.py), and on the device (the small model of
tests/test_gpu_svgd.py) the parameter block, every update tensor and the poses - launch by launch, through capture and replays, and in
the two-way PipelinedSampler.  Only names that every revision of sampler.py since the guidance terms has: run it once per tree in a
fresh process (LABEL names the tree, the lists are merged into out.json); two trees compute the same bits iff `check` finds their lists
equal.  A list holds one digest per job over the job's per-tensor digests; `tensors` keeps the per-tensor digests themselves, to find
the step and the tensor where two trees part."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GUIDED = dict(score_guidance_weight=0.5, score_guidance_max_tr=0.4, score_guidance_t_max=0.7)      # (t_max between two schedule points)
CONFIGS = {          # name -> (SamplerConfig fields, sample_slice of the 4 samples)
    "flexible": ({}, None),
    "rigid": (dict(flexible_sidechains=False), None),
    "ode": (dict(ode=True), None),
    "temp_sampling_1": (dict(temp_sampling=(1.0, 1.0, 1.0, 1.0)), None),
    "no_torsion": (dict(no_torsion=True), None),
    "no_final_step_noise": (dict(no_final_step_noise=True), None),
    "svgd_rigid": (dict(flexible_sidechains=False, svgd_weight=0.5, svgd_rot_rel_weight=0.7, svgd_tor_rel_weight=1.3, svgd_repulsive_weight=0.8), None),
    "clash_and_score_guidance": (dict(clash_guidance_weight=0.5, clash_guidance_max_tr=0.4, clash_guidance_t_max=0.7, **GUIDED), None),
    "score_guidance_sidechains": (dict(score_guidance_sidechains=True, **GUIDED), None),
    "record_trajectory": (dict(record_trajectory=True), None),
    "slice_1_3": ({}, slice(1, 3)),
}
N, SEED = 4, 3
out = {}


def put(name, tensors):
    for key, t in tensors.items():
        if t is not None:
            out[f"{name} {key}"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rolled_up(digests, depth):
    """One digest per job - the first `depth` words of a tensor's name: the configuration on the CPU, configuration and mode on the
    device - over the job's 'name digest' lines in sorted order, with their number: the form that is kept (a tenth of the size)."""
    jobs = {}
    for name in sorted(digests):
        jobs.setdefault(" ".join(name.split()[:depth]), []).append(f"{name} {digests[name]}")
    return {job: f"{hashlib.sha256(chr(10).join(lines).encode()).hexdigest()} ({len(lines)} tensors)" for job, lines in jobs.items()}


def run_cpu():
    from diffdock_pocket_amd import sampler as S
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from test_sampler_cpu import StubModel
    steps = 4
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20)
    T, n_sc = int(g["ligand"].edge_mask.sum()), int(g["flexResidues"].edge_idx.shape[0])
    sched = get_t_schedule(steps)
    for name, (fields, sl) in CONFIGS.items():
        smp = S.Sampler(StubModel(T, n_sc), g, N, torch.device("cpu"), S.SamplerConfig(inference_steps=steps, **fields), seed=SEED, sample_slice=sl)
        smp.randomize()
        put(f"{name} start", dict(lig_pos=smp.lig_pos, atom_pos=smp.atom_pos, gen=smp.gen.get_state()))
        for i in range(steps):
            smp.step(i, sched)
            put(f"{name} step{i}", dict(lig_pos=smp.lig_pos, atom_pos=smp.atom_pos, gen=smp.gen.get_state()))
        put(f"{name} end", dict(lig_traj=smp.lig_traj, atom_traj=smp.atom_traj))


def run_device():
    from diffdock_pocket_amd import sampler as S
    from diffdock_pocket_amd.diffusion import get_t_schedule
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from test_gpu_svgd import _model
    steps, dev = 5, torch.device("cuda:0")
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=16)
    sched = get_t_schedule(steps)

    def state(smp):
        return dict(params=smp.params, lig_pos=smp.lig_pos, atom_pos=smp.atom_pos, **{f"upd_{k}": v for k, v in smp.upd.items()})

    for name, (fields, sl) in CONFIGS.items():
        for mode in ("graph", "launches", "pipelined"):          # graph: two launch-by-launch steps, the capture, two replays
            if mode == "pipelined" and (fields.get("record_trajectory") or fields.get("svgd_weight")):
                continue                                         # (PipelinedSampler refuses both)
            cfg = S.SamplerConfig(inference_steps=steps, hip_graph=mode == "graph", **fields)
            if mode == "pipelined":
                smp = S.PipelinedSampler(_model(), g, N, dev, cfg, seed=SEED, sample_slice=sl, ways=2)
            else:
                smp = S.Sampler(_model(), g, N, dev, cfg, seed=SEED, sample_slice=sl)
            smp.randomize()
            for i in range(steps):
                smp.step(i, sched)
                torch.cuda.synchronize()
                tag = f"{name} {mode} step{i}"
                if mode == "pipelined":
                    put(tag, dict(lig_pos=smp.lig_pos, atom_pos=smp.atom_pos))
                    for k, part in enumerate(smp.parts):
                        put(f"{tag} part{k}", state(part))
                else:
                    put(tag, dict(gen=smp.gen.get_state(), **state(smp)))
            smp.check_overflow()
            if mode == "graph":
                assert smp._graph, f"{name}: the step was not captured"
                put(f"{name} {mode} end", dict(lig_traj=smp.lig_traj, atom_traj=smp.atom_traj))
                smp.close()


def check(path):
    with open(path) as f:
        data = json.load(f)
    labels = sorted(data)
    bad = 0
    for part in sorted(set().union(*(data[lb] for lb in labels))):
        lists = [data[lb][part]["sha256"] for lb in labels]
        diff = sorted(k for k in set().union(*lists) if len({ls.get(k) for ls in lists}) != 1)
        print(f"{part}: {len(lists[0])} digests, {len(labels)} trees ({', '.join(labels)}), {len(diff)} differ")
        for k in diff[:20]:
            print("  differs:", k)
        bad += len(diff)
    return 1 if bad or len(labels) < 2 else 0


if __name__ == "__main__":
    if sys.argv[1] == "check":
        sys.exit(check(sys.argv[2]))
    part, label, dst = sys.argv[1:4]
    with torch.no_grad():
        {"cpu": run_cpu, "device": run_device}[part]()
    data = {}
    if os.path.exists(dst):
        with open(dst) as f:
            data = json.load(f)
    info = {"sha256": out if "tensors" in sys.argv[4:] else rolled_up(out, 1 if part == "cpu" else 2)}
    if part == "device":
        info["device"] = torch.cuda.get_device_name(0)
    data.setdefault(label, {})[part] = info
    with open(dst, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
    print(len(out), f"digests of {label}/{part} ->", dst)
