"""Build libddp_hip.so in-tree for gfx950:  python -m diffdock_pocket_amd.build
(hipcc cross-compiles without a GPU; the .so is git-ignored but travels with the gpurun snapshot).

Every translation unit is compiled to its own object (cached under csrc/.obj/, keyed by the hash of the unit + the headers +
the flags), so that an edit of one kernel file recompiles that file only.  The library carries the SHA-256 of ALL its sources
as a tagged string (`DDP_SRC_SHA16=<16 hex digits>`, also returned by ddp_source_hash()): `built_hash` reads it from the file
bytes - no dlopen in the building process, so a stale library is never left loaded behind a rebuild."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = ["ddp_conv.hip", "ddp_conv_rows.hip", "ddp_conv_rows16.hip", "ddp_misc.hip", "ddp_gemm.hip", "ddp_pose.hip", "ddp_graph.hip", "ddp_views.hip", "ddp_lists.hip", "ddp_front_lists.hip", "ddp_node.hip", "ddp_heads.hip",
           "ddp_eval.hip", "ddp_traj.hip", "ddp_svgd.hip", "ddp_refine.hip", "ddp_guidance.hip", "ddp_score_guidance.hip", "ddp_score_guidance_flex.hip", "ddp_score.hip", "ddp_profile.hip", "ddp_minimize.hip", "ddp_minimize_flex.hip", "ddp_search.hip", "ddp_search_flex.hip", "ddp_pockets.hip", "ddp_capi.hip"]
HEADERS = [os.path.join(HERE, "csrc", "ddp_internal.h"), os.path.join(HERE, "csrc", "ddp_conv_diag.h"), os.path.join(HERE, "csrc", "ddp_conv_common.h"), os.path.join(HERE, "csrc", "ddp_conv_deal.h"), os.path.join(HERE, "csrc", "ddp_conv_rows_common.h"), os.path.join(HERE, "csrc", "ddp_horn.h"), os.path.join(HERE, "csrc", "ddp_pockets_uf.h"), os.path.join(HERE, "csrc", "ddp_score_pair.h"), os.path.join(HERE, "csrc", "ddp_pose_descent.h"), os.path.join(HERE, "csrc", "ddp_minimize_loop.h"), os.path.join(HERE, "csrc", "ddp_minimize_flex_loop.h"), os.path.join(HERE, "csrc", "ddp_clash_energy.h"), os.path.join(HERE, "csrc", "ddp_radius_math.h"),
           os.path.join(ROOT, "include", "ddp_hip.h")]
OUT = os.path.join(HERE, "libddp_hip.so")
OBJ_DIR = os.path.join(HERE, "csrc", ".obj")
_TAG = re.compile(rb"DDP_SRC_SHA16=([0-9a-f]{16})")


def _deps():
    return [os.path.join(HERE, "csrc", s) for s in SOURCES] + [h for h in HEADERS if os.path.exists(h)]


def source_hash():
    """16 hex digits of the SHA-256 over every source the library is compiled from, in a fixed order.  Compiled into the
    library (-DDDP_SRC_SHA16, exported as ddp_source_hash()) and checked by _lib.load(): the binary that runs is provably
    the one built from the sources in the tree."""
    h = hashlib.sha256()
    for d in _deps():
        h.update(os.path.basename(d).encode() + b"\0")
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_hash(path=None):
    """Source hash an existing library was built from (None if it is missing or carries no tag), read from the file."""
    path = path or OUT
    try:
        with open(path, "rb") as f:
            m = _TAG.search(f.read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def needs_build():
    """The library is rebuilt unless it carries the hash of the present sources (mtimes are not trusted: the .so travels to
    the GPU box with the snapshot)."""
    return built_hash() != source_hash()


# Per-unit compiler flags.  ddp_conv_rows.hip: without the SLP vectoriser - it packs the tile epilogues' fp32 FMAs into v_pk_fma_f32,
# which beside MFMAs cost more than the two v_fma_f32 they replace (MI355X guide, "packed f32 VALU ... an anti-lever beside MFMAs") and
# pushed the kernel from 0 to 6 spilled registers.  DDP_ROWS_SLP=1 in the environment keeps the vectoriser (same-box A/B builds).
EXTRA_FLAGS = {"ddp_conv_rows.hip": [] if os.environ.get("DDP_ROWS_SLP") else ["-fno-slp-vectorize"],
               "ddp_conv_rows16.hip": [] if os.environ.get("DDP_ROWS_SLP") else ["-fno-slp-vectorize"]}


def _compile(src, flags, verbose):
    """One translation unit -> cached object file."""
    flags = list(flags) + EXTRA_FLAGS.get(src, [])
    path = os.path.join(HERE, "csrc", src)
    h = hashlib.sha256(" ".join(flags).encode())
    for d in [path] + [x for x in HEADERS if os.path.exists(x)]:
        with open(d, "rb") as f:
            h.update(f.read())
    os.makedirs(OBJ_DIR, exist_ok=True)
    obj = os.path.join(OBJ_DIR, f"{os.path.splitext(src)[0]}.{h.hexdigest()[:16]}.o")
    if not os.path.exists(obj):
        for old in os.listdir(OBJ_DIR):      # one object per unit and flag set is enough
            if old.startswith(os.path.splitext(src)[0] + ".") and len(os.listdir(OBJ_DIR)) > 64:
                os.remove(os.path.join(OBJ_DIR, old))
        cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c"] + flags + \
              ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "csrc"), "-o", obj + ".tmp", path]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(obj + ".tmp", obj)
    return obj


def _link(out, defs, verbose):
    # the source hash is a define of ddp_capi.hip only: the other units' cached objects survive an edit elsewhere
    sha = f'-DDDP_SRC_SHA16="{source_hash()}"'
    flags = [f"-D{d}" for d in defs]
    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(lambda s: _compile(s, flags + ([sha] if s == "ddp_capi.hip" else []), verbose), SOURCES))
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


def build(force=False, verbose=True, stamps=False, ablate=0, defs=(), tag=""):
    """The product library, or a diagnostic variant that the product never loads (its name carries a suffix; loaded through
    DDP_HIP_LIB by the tools): `defs` = extra -D flags (library name suffixed with `tag`), stamps = in-kernel phase stamps
    (tools/stamp_conv.py), ablate = n: timing-only ablations whose results are wrong by construction (tools/ablate_conv.py).
    Every variant carries the source hash."""
    if defs:
        return _link(os.path.join(HERE, f"libddp_hip_{tag}.so"), list(defs), verbose)
    if ablate or stamps:
        out = os.path.join(HERE, "libddp_hip" + ("_stamps" if stamps else "") + (f"_ablate{ablate}" if ablate else "") + ".so")
        return _link(out, (["DDP_STAMPS"] if stamps else []) + ([f"DDP_ABLATE={ablate}"] if ablate else []), verbose)
    if not force and not needs_build():
        return OUT
    return _link(OUT, [], verbose)


if __name__ == "__main__":
    build(force="--force" in sys.argv, stamps="--stamps" in sys.argv)
