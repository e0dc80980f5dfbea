"""File output (diffdock_pocket_amd/outputs.py), trajectory recording of the CPU sampler, run_csv(out_dir=...) and the command line
(python -m diffdock_pocket_amd.inference), on the CPU with the stub score / confidence functions of test_inference_csv.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import outputs as O
from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.synthetic import make_3dpf_complex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLEX = "A:160-A:193-A:197"


def _texts():
    with open(os.path.join(GOLDEN, "3dpf_protein.pdb")) as f:
        pdb = f.read()
    with open(os.path.join(GOLDEN, "3dpf_ligand.sdf")) as f:
        sdf = f.read()
    return pdb, sdf


class Stub:
    """test_inference_csv.Stub: a deterministic pure function of the batch positions."""
    flexible_sidechains = True

    def __call__(self, b):
        B = b.num_graphs
        lp = b["ligand"].pos.reshape(B, -1, 3)
        c = lp.mean(1)
        tr = -0.05 * c
        rot = 0.02 * torch.stack([c[:, 1], -c[:, 0], c[:, 2]], 1)
        T = int(b["ligand"].edge_mask.sum())
        tor = 0.01 * lp[:, :1, 0].expand(B, T // B).reshape(-1) if T else torch.empty(0)
        S_ = b["flexResidues"].edge_idx.shape[0] if len(b["flexResidues"]) > 0 else 0
        sc = 0.01 * torch.ones(S_)
        return tr, rot, tor, sc


class StubConfidence:
    def __call__(self, b):
        B = b.num_graphs
        return -b["ligand"].pos.reshape(B, -1, 3).mean(1).norm(dim=1)


# ---------------------------------------------------------------------------------------------- writers
def test_sdf_round_trip_through_parse_sdf(tmp_path):
    _, sdf = _texts()
    heavy = I.remove_hs(I.parse_sdf(sdf))[0]
    g = I.build_complex_graph(*_texts())
    pos = g["ligand"].pos + 0.25                       # pocket-centred, moved
    path = O.write_sdf(str(tmp_path / "x.sdf"), heavy, pos, O.sdf_name(sdf), g.original_center)
    text = open(path).read()
    back = I.parse_sdf(text)
    assert text.splitlines()[0] == sdf.splitlines()[0] and text.rstrip().endswith("$$$$")
    assert back.elements == heavy.elements and back.bonds == heavy.bonds and back.charges == heavy.charges
    want = (pos + g.original_center).double().numpy()
    assert np.abs(back.pos - want).max() < 5e-5


def test_sdf_writes_formal_charges():
    mol = I.Molecule(np.zeros((3, 3)), ["N", "C", "O"], [(0, 1, 1), (1, 2, 1)], [1, 0, -1])
    back = I.parse_sdf(O.sdf_block(mol, np.arange(9.0).reshape(3, 3), "z"))
    assert back.charges == [1, 0, -1] and back.bonds == mol.bonds
    assert np.abs(back.pos - np.arange(9.0).reshape(3, 3)).max() == 0


def _flex_graph():
    pdb, sdf = _texts()
    return I.build_complex_graph(pdb, sdf, flexible_sidechains=FLEX), pdb


def test_receptor_writer_moves_only_the_side_chain_atoms(tmp_path):
    g, pdb = _flex_graph()
    moving = O.moving_atoms(g)
    assert moving.numel() > 0 and set(g.flex_atom_records) >= set(moving.tolist())
    shift = torch.tensor([0.5, -1.25, 2.0])
    new = g["atom"].pos[moving] + shift
    path = O.write_receptor(str(tmp_path / "r.pdb"), pdb, g, [new])
    out = open(path).read().splitlines()
    assert out[-1] == "END" and not any(ln.startswith("MODEL") for ln in out)
    recs = out[:-1]
    assert all(ln[:6] in ("ATOM  ", "HETATM") for ln in recs)
    assert not any(ln[76:78].strip() == "H" for ln in recs)
    # parse_pdb of the output: the moving atoms at their new place
    res = {(r.chain, r.resseq): r for r in I.parse_pdb("\n".join(out))}
    c = g.original_center.reshape(3)
    for node, p in zip(moving.tolist(), new):
        chain, _, resseq, _, name = g.flex_atom_records[node]
        got = torch.from_numpy(res[(chain, resseq)].atom(name).coord.astype(np.float32))
        assert float((got - (p + c)).abs().max()) < 5e-4
    # every other kept line is the input's, byte for byte; the changed lines differ in columns 31-54 only
    src = set(pdb.splitlines())
    changed = [ln for ln in recs if ln not in src]
    assert len(changed) == moving.numel()
    by_key = {(ln[:30], ln[54:]) for ln in pdb.splitlines()}
    assert all((ln[:30], ln[54:]) in by_key for ln in changed)
    heavy_in = [ln for ln in pdb.splitlines() if ln[:6] in ("ATOM  ", "HETATM") and ln[76:78].strip() != "H"]
    assert len(recs) == len(heavy_in)
    # the graph itself still goes into the model batch unchanged: the mapping is a graph-level attribute collate drops
    from diffdock_pocket_amd.batch import collate
    assert "flex_atom_records" not in collate([g, g])._globals


def test_receptor_trajectory_has_one_model_per_frame(tmp_path):
    g, pdb = _flex_graph()
    moving = O.moving_atoms(g)
    frames = [None, None] + [g["atom"].pos[moving] + 0.1 * k for k in range(4)]
    text = O.receptor_pdb(pdb, g.flex_atom_records, moving.tolist(), frames, g.original_center)
    lines = text.splitlines()
    assert sum(ln.startswith("MODEL") for ln in lines) == 6 and sum(ln == "ENDMDL" for ln in lines) == 6
    blocks = text.split("ENDMDL")[:-1]
    body = [b.strip().split("\n", 1)[1] for b in blocks]            # (without the MODEL line)
    assert body[0] == body[1] == body[2] != body[3]      # input, input, the input positions rewritten, then moved


def test_ligand_trajectory_models_and_conect(tmp_path):
    _, sdf = _texts()
    mol = O.heavy_molecule(sdf)
    g = I.build_complex_graph(*_texts())
    traj = torch.stack([g["ligand"].pos + k for k in range(5)])          # n_slots = 5
    path = O.write_ligand_trajectory(str(tmp_path / "t.pdb"), mol, O.ligand_frames(g["ligand"].pos, traj), g.original_center)
    text = open(path).read()
    models = text.split("ENDMDL")[:-1]
    assert len(models) == 5 + 2
    assert "CONECT" in models[0] and all("CONECT" not in m for m in models[1:])
    het = [ln for ln in models[3].splitlines() if ln.startswith("HETATM")]
    assert len(het) == len(mol.elements) and all(ln[17:26] == "UNL     1" for ln in het)
    assert [ln[76:78].strip() for ln in het] == [e.upper() for e in mol.elements]
    want = (traj[1] + g.original_center).numpy()
    got = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in het])
    assert np.abs(got - want).max() < 6e-4


# ---------------------------------------------------------------------------------------------- sampler
def _sampler(record, steps=4):
    g = make_3dpf_complex(seed=0, flexible_sidechains=True)
    T = int(g["ligand"].edge_mask.sum())
    S_ = g["flexResidues"].edge_idx.shape[0]

    class M:
        def __call__(self, b):
            B = b.num_graphs
            lp, ap = b["ligand"].pos.reshape(B, -1, 3), b["atom"].pos.reshape(B, -1, 3)
            c = lp.mean(1)
            return -0.05 * c, 0.02 * c, 0.01 * lp[:, :T, 0].reshape(-1), 0.01 * ap[:, :S_, 1].reshape(-1)

    cfg = S.SamplerConfig(inference_steps=steps, record_trajectory=record)
    return S.Sampler(M(), g, 3, "cpu", cfg, seed=5)


def test_cpu_sampler_records_every_step():
    steps = 4
    sch = get_t_schedule(steps)
    rec, ref = _sampler(True, steps), _sampler(False, steps)
    assert ref.lig_traj is None and ref.atom_traj is None
    rec.randomize()
    ref.randomize()
    moving = torch.unique(rec.sc_sub)
    assert rec.lig_traj.shape == (3, steps + 1, rec.n_l, 3) and rec.atom_traj.shape == (3, steps + 1, moving.numel(), 3)
    assert torch.equal(rec.lig_traj[:, 0], ref.lig_pos) and torch.equal(rec.atom_traj[:, 0], ref.atom_pos[:, moving])
    for t in range(steps):
        rec.step(t, sch)
        ref.step(t, sch)
        assert torch.equal(rec.lig_traj[:, t + 1], ref.lig_pos)
        assert torch.equal(rec.atom_traj[:, t + 1], ref.atom_pos[:, moving])
    assert torch.equal(rec.lig_pos, ref.lig_pos) and torch.equal(rec.atom_pos, ref.atom_pos)
    with pytest.raises(ValueError, match="outside"):
        rec.step(steps, np.concatenate([sch, sch]))


def test_restore_rewrites_slot_zero():
    s = _sampler(True, 2)
    s.randomize()
    snap = s.snapshot()
    s.run(get_t_schedule(2))
    s.lig_traj.zero_()
    s.restore(snap)
    assert torch.equal(s.lig_traj[:, 0], snap[0])


def test_pipelined_sampler_refuses_recording():
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    with pytest.raises(NotImplementedError):
        S.PipelinedSampler(Stub(), g, 4, "cpu", S.SamplerConfig(record_trajectory=True))


# ---------------------------------------------------------------------------------------------- run_csv + files
def _write_csv(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(
        "complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
        f"3dpf/flex,3dpf_protein.pdb,3dpf_ligand.sdf,,,,{FLEX}\n"
        "3dpf_smiles,3dpf_protein.pdb,COc(cc1)ccc1C#N\n"
        "3dpf_rigid,3dpf_protein.pdb,3dpf_ligand.sdf\n")
    return str(p)


def _run(csv_path, out_dir, rank=0, world=1, dist=None, conf=True, vis=True):
    return INF.run_csv(csv_path, Stub(), torch.device("cpu"), confidence_model=StubConfidence() if conf else None, samples_per_complex=5,
                       inference_steps=3, root=GOLDEN, seed=2, rank=rank, world=world, dist=dist, allow_zero_esm=True,
                       out_dir=out_dir, save_visualisation=vis)


def test_run_csv_writes_ranked_files(tmp_path):
    out = str(tmp_path / "out")
    res = _run(_write_csv(tmp_path), out)
    assert res[1].skipped is not None and res[1].files == []
    flex, rigid = res[0], res[2]
    d = os.path.join(out, "index0___3dpf-flex")
    assert os.path.isdir(d) and os.path.isdir(os.path.join(out, "index2___3dpf_rigid"))
    conf = flex.confidence
    names = {os.path.basename(p) for p in flex.files}
    want = {"rank1.sdf", "rank1_protein.pdb"}
    for k in range(5):
        want |= {f"rank{k + 1}_confidence{float(conf[k]):.2f}.sdf", f"rank{k + 1}_confidence{float(conf[k]):.2f}_protein.pdb",
                 f"rank{k + 1}_reverseprocess.pdb", f"rank{k + 1}_reverseprocess_protein.pdb"}
    assert names == want and set(os.listdir(d)) == want
    assert not any("protein" in os.path.basename(p) for p in rigid.files)
    # rank k's SDF holds the k-th ranked pose
    oc = flex.original_center.reshape(1, 3)
    for k in range(5):
        back = I.parse_sdf(open(os.path.join(d, f"rank{k + 1}_confidence{float(conf[k]):.2f}.sdf")).read())
        assert np.abs(back.pos - (flex.ligand_pos[k].double() + oc.double()).numpy()).max() < 5e-5
    assert open(os.path.join(d, "rank1.sdf")).read() == open(os.path.join(d, f"rank1_confidence{float(conf[0]):.2f}.sdf")).read()
    # trajectories in ranked order: the last slot is the returned pose
    assert flex.lig_traj.shape[:2] == (5, 4) and torch.equal(flex.lig_traj[:, -1], flex.ligand_pos)
    assert flex.atom_traj is not None and rigid.atom_traj is None
    last = open(os.path.join(d, "rank2_reverseprocess.pdb")).read().split("ENDMDL")[-2]
    het = [ln for ln in last.splitlines() if ln.startswith("HETATM")]
    got = np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in het])
    assert np.abs(got - (flex.ligand_pos[1] + oc).numpy()).max() < 6e-4


def test_run_csv_without_confidence_and_without_out_dir(tmp_path):
    out = str(tmp_path / "out")
    res = _run(_write_csv(tmp_path), out, conf=False, vis=False)
    names = {os.path.basename(p) for p in res[2].files}
    assert names == {f"rank{k + 1}.sdf" for k in range(5)}
    assert res[2].lig_traj is None
    plain = INF.run_csv(_write_csv(tmp_path), Stub(), torch.device("cpu"), samples_per_complex=5, inference_steps=3, root=GOLDEN,
                        seed=2, allow_zero_esm=True)
    assert plain[2].files == [] and torch.equal(plain[2].ligand_pos, res[2].ligand_pos)


def _worker(rank, world, csv_path, out_dir, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _run(csv_path, out_dir, rank, world, dist)
    q.put((rank, [(r.name, r.skipped, [os.path.basename(p) for p in r.files]) for r in res]))
    dist.barrier()
    dist.destroy_process_group()


def _tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_two_rank_run_writes_the_single_process_files(tmp_path):
    csv_path = _write_csv(tmp_path)
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _run(csv_path, one)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, csv_path, two, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(files == [] for _, _, files in got[1])          # rank 1 writes nothing
    a, b = _tree(one), _tree(two)
    assert len(a) > 0 and a.keys() == b.keys()
    assert all(a[k] == b[k] for k in a)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_reports_argument_errors(tmp_path, capsys):
    pdb = os.path.join(GOLDEN, "3dpf_protein.pdb")
    with pytest.raises(SystemExit) as e:
        INF.main(["--protein_path", pdb, "--ligand", os.path.join(GOLDEN, "3dpf_ligand.sdf"), "--model_dir", str(tmp_path / "none")])
    assert e.value.code == 2 and "model_parameters.yml" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        INF.main(["--protein_path", pdb, "--ligand", os.path.join(GOLDEN, "3dpf_ligand.sdf")])
    assert e.value.code == 2 and "--model_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        INF.main(["--protein_path", pdb, "--protein_ligand_csv", _write_csv(tmp_path), "--model_dir", str(tmp_path)])
    assert e.value.code == 2 and "not both" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        INF.main(["--model_dir", str(tmp_path)])
    assert e.value.code == 2
