"""Case tables of tests/test_gpu_list_seams.py: inputs only, numpy, no device (tests/test_lists_ref_cpu.py checks that they are
well formed).  A case is a plain dict of sizes and int32-ranged arrays; `odd` names the one array whose device view starts
4 bytes off 16-byte alignment (None: every view aligned)."""
import numpy as np

MAX_JOBS = 12               # DDP_MAX_LIST_JOBS: the wrappers split longer job lists into launches of 12
SCAN_SMALL_MAX = 49152      # ddp_scan_jobs takes its small form when EVERY job of the launch has a capacity of at most this
SCAN_MODES = ("ones", "flag_list", "val_excl2", "flag_val", "flag_rowptr", "val_inplace")
# outputs a mode hands to the kernel ("val_inplace": excl2 IS val, the aliasing ddp_group_by_key_jobs uses)
SCAN_OUTPUTS = {"ones": ("excl", "excl2", "list", "total"), "flag_list": ("excl", "list", "total"),
                "val_excl2": ("excl", "excl2", "total"), "flag_val": ("excl2", "total"), "flag_rowptr": ("excl", "total"),
                "val_inplace": ("excl", "excl2", "total")}
SCAN_ODD = {"ones": ("excl", "excl2"), "flag_list": ("flag", "excl"), "val_excl2": ("in", "excl", "excl2"),
            "flag_val": ("in", "flag", "excl2"), "flag_rowptr": ("in", "flag", "excl"), "val_inplace": ("in", "excl")}
SCAN_SIZES = (1, 3, 0, 4, 5, 255, 256, 257, 4095, 4096, 4097, 49151, 49152)      # (the empty job sits between live ones)
SCAN_LARGE = (49153, 53248, 53249, 100003)


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _counts(n, kind):
    """(capacity, device-side count or None) of a job whose actual count is n."""
    return {"none": (n, None), "eq": (n, n), "slack": (n + 37, n), "over": (n, n + 5)}[kind]


def scan_segment(n):
    """Items per wave of the scan kernels: ceil(ceil(n / 16) / 256) * 256."""
    return -(-(-(-n // 16)) // 256) * 256


def scan_case(seed, mode, n, kind="none", base=0, odd=None, neg=False):
    rng = _rng(1, seed)
    cap, n_dev = _counts(n, kind)
    if neg:
        n_dev = -3                                              # treated as 0
    m = max(cap, 1)
    flag = (rng.random(m) < 0.3).astype(np.int64)
    val = rng.integers(0, 9, m)
    lens = rng.integers(0, 9, m)                                # rows of length 0 included
    S = scan_segment(n)
    if S and n >= 2 * S:                                        # a run of zeros covering wave 1's whole segment
        flag[S:2 * S] = 0
        val[S:2 * S] = 0
    if S and n >= 3 * S:
        lens[2 * S:3 * S] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    c = dict(mode=mode, cap=cap, n_dev=n_dev, base=base, odd=odd, n=0 if neg else n)
    if mode in ("flag_list", "flag_val", "flag_rowptr"):
        c["flag"] = flag
    if mode in ("val_excl2", "flag_val", "val_inplace"):
        c["val"] = val
    if mode == "flag_rowptr":
        c["rowptr"] = rowptr
    return c


def _scan_groups(jobs, form, seed):
    """Launches of exactly MAX_JOBS jobs (the last may be shorter).  General form: every launch also holds one job of capacity
    SCAN_SMALL_MAX + 1, at a varying place, which switches the whole launch to ddp_scan_jobs_kernel."""
    if form == "small":
        return [jobs[i:i + MAX_JOBS] for i in range(0, len(jobs), MAX_JOBS)]
    groups = []
    for g, i in enumerate(range(0, len(jobs), MAX_JOBS - 1)):
        part = list(jobs[i:i + MAX_JOBS - 1])
        trig = scan_case(seed + 7000 + g, SCAN_MODES[g % 6], SCAN_SMALL_MAX + 1, base=11 * (g % 2))
        if g % 3:
            trig["n_dev"], trig["n"] = 7, 7                    # the capacity decides the form, not the count
        part.insert((5 * g) % (len(part) + 1), trig)
        groups.append(part)
    return groups


def scan_sweep(form):
    """Every mode x every seam size, device-side counts and bases rotating; form 'small' or 'general'."""
    kinds = ("none", "slack", "over", "eq")
    jobs = []
    for mi, mode in enumerate(SCAN_MODES):
        for si, n in enumerate(SCAN_SIZES):
            kind = kinds[(mi + si) % 4]
            if form == "small" and kind == "slack" and n + 37 > SCAN_SMALL_MAX:
                kind = "eq"
            jobs.append(scan_case(100 * mi + si, mode, n, kind, base=11 * ((mi + si) % 2)))
    jobs.insert(30, scan_case(901, "flag_list", 300, neg=True))
    jobs.insert(50, scan_case(902, "val_excl2", 4097, base=11, neg=True))
    return _scan_groups(jobs, form, 1)


def scan_large():
    """Sizes only the general form serves: 13 full chunks per wave (53248 = 16 x 3328), one item more, and a ragged 100003."""
    kinds = ("none", "slack", "over")
    jobs = [scan_case(2000 + 10 * mi + si, mode, n, kinds[(mi + si) % 3], base=11 * ((mi + si) % 2))
            for mi, mode in enumerate(SCAN_MODES) for si, n in enumerate(SCAN_LARGE)]
    return [jobs[i:i + MAX_JOBS] for i in range(0, len(jobs), MAX_JOBS)]


def scan_scalar(form):
    """One array of the job on a view 4 bytes off 16-byte alignment: the whole job takes the scalar loads and stores."""
    jobs = []
    for mi, mode in enumerate(SCAN_MODES):
        for oi, odd in enumerate(SCAN_ODD[mode]):
            for si, n in enumerate((3, 4, 5, 257, 4097)):
                jobs.append(scan_case(3000 + 100 * mi + 10 * oi + si, mode, n, ("none", "slack", "over")[(oi + si) % 3],
                                      base=11 * ((oi + si) % 2), odd=odd))
        jobs.append(scan_case(3900 + mi, mode, SCAN_SMALL_MAX if form == "small" else 53249, base=11 * (mi % 2), odd=SCAN_ODD[mode][-1]))
    return _scan_groups(jobs, form, 2)


def scan_form(group):
    """The kernel's own rule (ddp_scan_jobs)."""
    return "small" if all(c["cap"] <= SCAN_SMALL_MAX for c in group) else "general"


# ------------------------------------------------------------------------------------------------ select
SELECT_SIZES = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 6145)
SELECT_FLAGS = ("all", "none", "some", "last", "block_first")
SELECT_FORMS = ("ab_idx", "a_only", "b_idx", "a_bidx")
N_NODES = 97


def select_case(seed, cap, n_dev, flags, form, n_pay=2, drop_out=(), out_idx=True, pay_add=None, total0=9):
    """Masks and index lists that give the wanted per-item flags in the wanted form; payloads; `drop_out`: payloads whose
    output is absent."""
    rng = _rng(2, seed)
    m = max(cap, 1)
    i = np.arange(m)
    f = {"all": np.ones(m, bool), "none": np.zeros(m, bool), "some": rng.random(m) < 0.3, "last": i == cap - 1,
         "block_first": i % 2048 == 0}[flags]
    c = dict(cap=cap, n_dev=n_dev, flags=flags, form=form, out_idx=out_idx, drop_out=tuple(drop_out), total0=total0,
             pay_add=list(pay_add) if pay_add is not None else None, mask_a=None, idx_a=None, mask_b=None, idx_b=None)
    node_mask = np.zeros(N_NODES, dtype=np.int64)
    node_mask[rng.permutation(N_NODES)[:30]] = rng.integers(1, 4, 30)            # (any nonzero value flags)
    on, offn = np.nonzero(node_mask)[0], np.nonzero(node_mask == 0)[0]

    def indexed(want):
        return np.where(want, on[rng.integers(0, on.shape[0], m)], offn[rng.integers(0, offn.shape[0], m)])

    if form == "a_only":
        c["mask_a"] = f.astype(np.int64) * rng.integers(1, 4, m)
    elif form == "b_idx":
        c["mask_b"], c["idx_b"] = node_mask, indexed(f)
    else:
        in_a = f & (rng.random(m) < 0.6)
        in_b = (f & ~in_a) | (f & (rng.random(m) < 0.3))
        c["mask_b"], c["idx_b"] = node_mask, indexed(in_b)
        if form == "a_bidx":
            c["mask_a"] = in_a.astype(np.int64)
        else:
            c["mask_a"], c["idx_a"] = node_mask[::-1].copy(), N_NODES - 1 - indexed(in_a)
    c["pays"] = [rng.integers(-1000, 100000, m) for _ in range(n_pay)]
    return c


def select_sweep():
    jobs = []
    for si, n in enumerate(SELECT_SIZES):
        for fi, flags in enumerate(SELECT_FLAGS):
            q = si + fi
            n_pay = 1 + q % 4
            jobs.append(select_case(10 * si + fi, n, (None, n)[q % 2], flags, SELECT_FORMS[q % 4], n_pay,
                                    drop_out=[k for k in range(n_pay) if (q + k) % 3 == 2], out_idx=q % 5 != 4,
                                    pay_add=[(0, 5, -7, 1 << 20)[(q + k) % 4] for k in range(n_pay)] if q % 3 else None))
    jobs.append(select_case(500, 6145, 2048, "some", "ab_idx", 4))               # two wholly empty blocks behind the count
    jobs.append(select_case(501, 6145, 2049, "all", "a_only", 0))                # pockets.py's form: the kept indices only
    jobs.append(select_case(502, 513, 0, "all", "ab_idx", 3))
    jobs.append(select_case(503, 2049, 0, "some", "b_idx", 1))
    jobs.append(select_case(504, 2047, 2047 + 9, "all", "a_bidx", 2, pay_add=[3, 0]))
    jobs.append(select_case(505, 65, 1 << 30, "some", "ab_idx", 1))
    return jobs


def select_tables():
    """Calls of the wrapper: 12 live jobs of different sizes (one launch), 13 jobs (split), and jobs with n == 0 first, in the
    middle and last, each with a total of its own."""
    twelve = [select_case(600 + k, n, (None, n - n // 3)[k % 2], SELECT_FLAGS[k % 5] if k % 5 != 1 else "some", SELECT_FORMS[k % 4], 1 + k % 3)
              for k, n in enumerate((1, 2049, 64, 6145, 513, 65, 4096, 2047, 511, 2048, 63, 4097))]
    thirteen = [select_case(700 + k, n, None, "some", SELECT_FORMS[(k + 1) % 4], 1 + k % 4)
                for k, n in enumerate((2049, 1, 513, 64, 4096, 63, 2048, 65, 511, 6145, 512, 2047, 130))]
    empties = [select_case(800, 0, None, "all", "a_only", 1, total0=5),
               select_case(801, 2049, None, "some", "ab_idx", 2),
               select_case(802, 0, None, "all", "ab_idx", 0, total0=6),
               select_case(803, 513, 300, "some", "b_idx", 1),
               select_case(804, 0, 4, "all", "a_only", 1, total0=7)]
    return [twelve, thirteen, empties]


# ------------------------------------------------------------------------------------------------ mark
MARK_MASK = 400


def mark_calls():
    """Launches of three jobs with an empty one in the middle; mask names: jobs with the same name write into one mask."""
    rng = _rng(3)

    def job(mask, n, n_dev=None, idx=True, repeat=False):
        m = max(n, 1)
        ix = rng.integers(0, 20 if repeat else MARK_MASK, m) if idx else None
        return dict(mask=mask, n=n, n_dev=n_dev, idx=ix)

    return [[job("m0", 1), job("m1", 0), job("m2", 255)],
            [job("m3", 256), job("m4", 0, n_dev=3), job("m5", 257, repeat=True)],
            [job("m6", 257, idx=False), job("m7", 0), job("m8", 256, n_dev=255)],
            [job("m9", 300, n_dev=0), job("m10", 0), job("m11", 257, n_dev=999, idx=False)],
            [job("shared", 255, repeat=True), job("m12", 0), job("shared", 257, n_dev=200)],
            [job("m13", 1, idx=False), job("m14", 0), job("m15", 255, n_dev=-3)]]


# ------------------------------------------------------------------------------------------------ rowcopy
ROW_LENGTHS = (0, 1, 63, 64, 65, 130, 200)


def rowcopy_calls():
    rng = _rng(4)
    jobs = []
    for ri, n_rows in enumerate((1, 3, 4, 5, 129)):
        for ki, keep_kind in enumerate(("all", "none", "random", "ends")):
            lens = np.asarray(ROW_LENGTHS)[rng.integers(0, len(ROW_LENGTHS), n_rows)]
            if n_rows == 1:
                lens[:] = ROW_LENGTHS[3 + ki % 4]
            keep = {"all": np.full(n_rows, 2), "none": np.zeros(n_rows, dtype=np.int64), "random": (rng.random(n_rows) < 0.5).astype(np.int64),
                    "ends": np.zeros(n_rows, dtype=np.int64)}[keep_kind]
            if keep_kind == "ends":
                keep[0] = keep[-1] = 1
            old = np.concatenate([[0], np.cumsum(lens)])
            e = max(int(old[-1]), 1)
            jobs.append(dict(n_rows=n_rows, keep=keep, old_rowptr=old, n_edges=int(old[-1]), ins=[rng.integers(0, 1 << 20, e) for _ in range(1 + (ri + ki) % 3)]))
    empty = dict(n_rows=0, keep=np.zeros(1, dtype=np.int64), old_rowptr=np.zeros(1, dtype=np.int64), n_edges=0, ins=[np.zeros(1, dtype=np.int64)])
    return [jobs[:5] + [empty] + jobs[5:11], jobs[11:14] + [empty] + jobs[14:]]


# ------------------------------------------------------------------------------------------------ gather_rows
def _float_bits(rng, shape):
    """fp32 bit patterns with NaN payloads and signed zeros among ordinary values."""
    x = rng.standard_normal(shape).astype(np.float32).view(np.int32).astype(np.int64)
    r = rng.random(shape)
    x = np.where(r < 0.05, np.int64(0x7fc00000) + rng.integers(1, 1 << 20, shape), x)            # quiet NaNs with payloads
    x = np.where((r >= 0.05) & (r < 0.08), np.int64(0x7f800001) + rng.integers(0, 1 << 20, shape), x)   # signalling NaNs
    x = np.where((r >= 0.08) & (r < 0.12), np.int64(-0x80000000), x)                             # -0.0
    x = np.where((r >= 0.12) & (r < 0.14), 0, x)
    return x.astype(np.int64)


def gather_cases():
    rng = _rng(5)
    cases = []
    for ci, ncols in enumerate((1, 63, 64, 65, 130)):
        for ni, n in enumerate((1, 3, 4, 5, 301)):
            n_dev = (None, n - 1 if n > 1 else 0, 0, n + 3)[(ci + ni) % 4]
            cases.append(dict(ncols=ncols, n=n, n_dev=n_dev, rows=50, ldx=ncols + 3, ldo=ncols + 5,
                              x=_float_bits(rng, (50, ncols + 3)), idx=rng.integers(0, 50 if n > 5 else 2, n)))
    return cases


# ------------------------------------------------------------------------------------------------ clean_pair_maps
def clean_case(seed, B, n0, e0, with_rowptr, p_touch=0.3):
    """B samples of n0 atoms with e0 edges each in receiver-CSR order.  Without rowptr every sample has sample 0's list.  With
    rowptr the touched receivers of a sample trade row lengths among themselves (the sample keeps e0 edges; an untouched
    receiver keeps the row length of its copy in sample 0)."""
    rng = _rng(6, seed)
    touched = (rng.random((B, n0)) < p_touch).astype(np.int64) * rng.integers(1, 3, (B, n0))
    touched[:, 3 % n0] = 1                                      # touched in every sample: rows_v falls back to g = 0
    if n0 > 5:
        touched[0, 5] = 1                                       # first untouched sample is not sample 0
        touched[1:, 5] = 0
    len0 = rng.multinomial(e0, np.full(n0, 1.0 / n0))
    lens = np.tile(len0, (B, 1))
    if with_rowptr:
        for s in range(1, B):                                   # (sample 0 holds the reference rows)
            t = np.nonzero(touched[s])[0]
            for _ in range(4 * len(t) if len(t) > 1 else 0):
                i, j = rng.choice(t, 2, replace=False)
                if lens[s, i] > 0:
                    lens[s, i] -= 1
                    lens[s, j] += 1
    recv = np.repeat(np.arange(B * n0), lens.reshape(-1))
    src = rng.integers(0, n0, B * e0) + (np.arange(B * e0) // e0) * n0
    if not with_rowptr:
        src = np.tile(src[:e0], B) + (np.arange(B * e0) // e0) * n0
    rowptr = np.concatenate([[0], np.cumsum(lens.reshape(-1))])
    return dict(B=B, n0=n0, e0=e0, E=B * e0, touched=touched.reshape(-1), recv=recv, src=src, rowptr=rowptr if with_rowptr else None)


def clean_cases():
    shapes = ((5, 40, 130), (2, 300, 100), (2, 50, 128), (1, 30, 257), (1, 300, 256), (3, 7, 86))   # (B, n0, e0): E < n0, E = 256, 257, B = 1
    return [clean_case(10 * k + w, B, n0, e0, bool(w)) for k, (B, n0, e0) in enumerate(shapes) for w in (0, 1)]


# ------------------------------------------------------------------------------------------------ flex_mark / fallback_rowmap
NEG_ZERO = -0x80000000


def flex_case(seed, B, n_a, n_b, e0, a_too, ref_list, how):
    """how: 'moved' (a few atoms displaced), 'ulp' (one coordinate one ulp away), 'zero' (-0.0 where sample 0 has +0.0),
    'flag' (an earlier pass's mask instead of positions)."""
    rng = _rng(7, seed)
    pos0 = rng.standard_normal((n_b, 3)).astype(np.float32)
    pos0[::4, 1] = 0.0                                          # +0.0 coordinates
    pos = np.tile(pos0.view(np.int32).astype(np.int64), (B, 1, 1))
    moved = rng.random((B, n_b)) < 0.1
    moved[0] = False
    if how == "moved":
        pos[moved] += 1 << 12
    elif how == "ulp":
        pos[:, :, 2][moved] += 1
    elif how == "zero":
        moved[:, np.arange(n_b) % 4 != 0] = False
        moved[1:, 0] = True
        pos[:, :, 1][moved] = NEG_ZERO
    flag = (rng.random((B, n_b)) < 0.15).astype(np.int64) * rng.integers(1, 3, (B, n_b)) if how == "flag" else None
    offs_a, offs_b = (np.arange(B) * n_a)[:, None], (np.arange(B) * n_b)[:, None]
    a = (np.sort(rng.integers(0, n_a, (B, e0)), axis=1) + offs_a).reshape(-1)
    b = (rng.integers(0, n_b, (B, e0)) + offs_b).reshape(-1)
    return dict(B=B, n_a=n_a, n_b=n_b, e0=e0, n_edges=B * e0, a_too=a_too, ref_list=ref_list, how=how, a=a, b=b,
                pos=None if how == "flag" else pos.reshape(-1, 3), flag=None if flag is None else flag.reshape(-1),
                off=(flag.reshape(B, n_b) != 0) if how == "flag" else moved)


def flex_cases():
    cases, k = [], 0
    for how in ("moved", "ulp", "zero", "flag"):
        for B, n_a, n_b, e0, a_too, ref_list in ((4, 23, 57, 200, False, False), (4, 23, 57, 200, False, True),   # receptor<-atom shape
                                                 (2, 300, 300, 50, True, True),                                    # n_edges < n_a_per_graph
                                                 (2, 57, 57, 128, True, False), (1, 57, 57, 257, True, True), (3, 57, 57, 86, True, True)):
            cases.append(flex_case(k, B, n_a, n_b, e0, a_too, ref_list, how))
            k += 1
    return cases


def fallback_case(seed, B, n, n_edges):
    """Marked receivers with row lengths of their own, unmarked ones with their sample-0 copy's; sample 0 wholly marked."""
    rng = _rng(8, seed)
    mark = (rng.random((B, n)) < 0.4).astype(np.int64)
    mark[0] = 1
    hi = 7 if n_edges >= 3 * B * n else 1                       # (few edges: start from empty rows and only add)
    lens = np.tile(rng.integers(0, hi, n), (B, 1))
    lens[1:][mark[1:] != 0] = rng.integers(0, hi, int((mark[1:] != 0).sum()))
    lens = lens.reshape(-1)
    marked = np.nonzero(mark.reshape(-1))[0]
    copied = np.unique(np.nonzero(mark.reshape(-1) == 0)[0] % n)            # sample-0 rows that unmarked receivers copy
    free = np.setdiff1d(marked, copied)                                     # rows whose length binds no other row's
    assert free.shape[0] > 0
    for _ in range(100000):
        d = n_edges - int(lens.sum())
        if d == 0:
            break
        r = free[rng.integers(0, free.shape[0])]
        lens[r] += 1 if d > 0 else -min(1, lens[r])
    assert lens.sum() == n_edges
    old = np.concatenate([[0], np.cumsum(lens)])
    new = np.concatenate([[0], np.cumsum(lens * (mark.reshape(-1) != 0))])
    return dict(B=B, n=n, n_edges=n_edges, mark=mark.reshape(-1), recv=np.repeat(np.arange(B * n), lens), old_rowptr=old, new_rowptr=new)


def fallback_cases():
    return [fallback_case(0, 1, 1, 1), fallback_case(1, 3, 20, 255), fallback_case(2, 3, 20, 257), fallback_case(3, 2, 9, 1)]


# ------------------------------------------------------------------------------------------------ group_by_key
def group_case(seed, n_items, n_dev, n_keys, keys="random", n_pay=2, drop_out=(), key_map=False, perm=True, odd_rowptr=False, out_key=True):
    rng = _rng(9, seed)
    m = max(n_items, 1)
    if keys == "random":
        key = rng.integers(0, n_keys, m)
    elif keys == "one":
        key = np.full(m, n_keys // 2)
    elif keys == "inner":                                        # empty first and last keys
        key = rng.integers(1, n_keys - 1, m)
    else:                                                        # rows of exactly these lengths, shuffled; first and last key empty
        key = rng.permutation(np.repeat(np.arange(1, 1 + len(keys)), keys))
        assert key.shape[0] == n_items and n_keys == len(keys) + 2
    return dict(n_items=n_items, n_dev=n_dev, n_keys=n_keys, key=key, pays=[rng.integers(0, 1 << 20, m) for _ in range(n_pay)],
                drop_out=tuple(drop_out), key_map=rng.permutation(n_keys) if key_map else None, perm=perm, odd_rowptr=odd_rowptr,
                out_key=out_key and perm)


def group_calls():
    """(form, jobs) per launch; the form follows from the largest n_keys of the launch (the scan runs in place over the keys)."""
    small = [group_case(0, 300, 255, 1, n_pay=1), group_case(1, 300, 256, 255, key_map=True),
             group_case(2, 300, 257, 256, n_pay=3, drop_out=(1,)), group_case(3, 300, 0, 257),
             group_case(4, 395, None, 5, keys=(65, 130, 200), key_map=True, odd_rowptr=True),
             group_case(5, 0, None, 9, n_pay=1),                                             # an empty job between live ones
             group_case(6, 3000, None, 3, keys="one", n_pay=1), group_case(7, 20000, 19999, SCAN_SMALL_MAX, n_pay=0, out_key=False),
             group_case(8, 5000, None, 70, perm=False), group_case(9, 700, 600, 257, keys="inner", n_pay=3, drop_out=(0, 2)),
             group_case(10, 257, None, 256, perm=False, odd_rowptr=True), group_case(11, 1000, None, 255, n_pay=2, drop_out=(0,), odd_rowptr=True)]
    general = [group_case(20, 20000, None, SCAN_SMALL_MAX + 1, n_pay=1), group_case(21, 300, 256, 255, key_map=True),
               group_case(22, 0, None, 4), group_case(23, 30000, 29000, 60000, key_map=True, n_pay=3),
               group_case(24, 395, None, 5, keys=(65, 130, 200), odd_rowptr=True), group_case(25, 5000, None, 60000, perm=False),
               group_case(26, 300, 257, 256), group_case(27, 40, None, 1, n_pay=1),
               group_case(28, 9000, None, 4097, keys="inner", odd_rowptr=True), group_case(29, 257, 0, 257),
               group_case(30, 2000, None, SCAN_SMALL_MAX + 1, perm=False, odd_rowptr=True), group_case(31, 1000, 255, 300, n_pay=2)]
    return [("small", small), ("general", general)]


def group_form(jobs):
    return "small" if all(c["n_keys"] <= SCAN_SMALL_MAX for c in jobs) else "general"
