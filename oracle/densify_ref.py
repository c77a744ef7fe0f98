"""Independent numpy restatement of the densification cycle (the spec at the top of csrc/densify.hip), for the tests only.

Every decision is made in fp32, as torch makes it on fp32 tensors: g = accum / denom with NaN -> 0, |g| >= threshold,
smax = max exp(s), sigmoid(o) = 1 / (1 + exp(-o)).  The thresholds are formed in double and rounded to fp32 once (torch
comparing an fp32 tensor with a Python float).  numpy's fp32 exp / log are not the device's expf / logf: the two may
differ by an ulp, so the inputs these tests decide on keep away from every threshold (`synthetic_state`).

Results are the selection masks over the N sources and the row map of the result as (src, slot): slot 0 original,
1 clone, 2 / 3 first / second child, in the reference's order (originals neither split nor pruned, kept clones, kept
first children, kept second children; source order inside each).  The children's xyz and scaling are formed in float64.
"""
import numpy as np

SPLIT_DIV = np.float32(0.8 * 2)  # densify_and_split divides by 0.8 * N with N = 2
RESET_CAP = np.float32(0.01)

# synthetic_state's row categories
KEEP, CLONE, SPLIT, PRUNED, CHILD_PRUNED = 0, 1, 2, 3, 4
SCALE_MARGIN, OPACITY_MARGIN = 1e-5, 1e-6  # relative, as tests/golden/make_densify_golden.py


def _sigmoid32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-x))


def _thresholds(grad_threshold, percent_dense, extent, min_opacity, max_screen_size):
    return dict(grad=np.float32(grad_threshold), split=np.float32(percent_dense * extent),
                min_op=np.float32(min_opacity), world=np.float32(0.1 * extent),
                screen=np.float32(max_screen_size or 0.0), size=bool(max_screen_size))


def classify(scaling, opacity, accum, denom, *, grad_threshold, percent_dense, extent, min_opacity, max_screen_size=None):
    """Per-source decisions of densify_and_prune: dict of bool [N] arrays clone, split, prune (the original or its clone
    goes), child_prune (a split source's children go), keep, clone_kept, children_kept."""
    t = _thresholds(grad_threshold, percent_dense, extent, min_opacity, max_screen_size)
    s = np.asarray(scaling, np.float32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.asarray(accum, np.float32).reshape(-1) / np.asarray(denom, np.float32).reshape(-1)
    g[np.isnan(g)] = np.float32(0.0)
    sel = np.abs(g) >= t["grad"]
    with np.errstate(over="ignore"):
        smax = np.exp(s).max(axis=1)
        cmax = np.exp(np.log(np.exp(s) / SPLIT_DIV)).max(axis=1)
    clone = sel & (smax <= t["split"])
    split = sel & (smax > t["split"])
    op = _sigmoid32(np.asarray(opacity, np.float32).reshape(-1))
    # max_radii2D is read after densification_postfix zeroed it: 0 > max_screen_size
    vs = t["size"] and bool(np.float32(0.0) > t["screen"])
    low = (op < t["min_op"]) | vs
    prune = low | (t["size"] & (smax > t["world"]))
    child_prune = split & (low | (t["size"] & (cmax > t["world"])))
    return dict(clone=clone, split=split, prune=prune, child_prune=child_prune, keep=~split & ~prune,
                clone_kept=clone & ~prune, children_kept=split & ~child_prune)


def _row_map(segments):
    src = np.concatenate([np.flatnonzero(m) for m in segments]).astype(np.int64)
    slot = np.concatenate([np.full(int(m.sum()), k, np.int8) for k, m in enumerate(segments)])
    return src, slot


def cat_prune(c):
    """The final prune mask over the reference's concatenated set (originals not split, clones, first and second
    children)."""
    return np.concatenate([c["prune"][~c["split"]], c["prune"][c["clone"]], c["child_prune"][c["split"]],
                           c["child_prune"][c["split"]]])


def children(xyz, scaling, rotation, noise, src, slot):
    """xyz and scaling of the child rows (slot >= 2) of a row map, in float64: R(normalize(q)) (z (.) exp(s)) + xyz and
    log(exp(s) / 1.6), with z = noise[src, slot - 2] (noise: [N, 2, 3], standard normal)."""
    ch = slot >= 2
    i, copy = src[ch], slot[ch].astype(np.int64) - 2
    s = np.asarray(scaling, np.float32)[i].astype(np.float64)
    q = np.asarray(rotation, np.float32)[i].astype(np.float64)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    zz = np.asarray(noise, np.float32)[i, copy].astype(np.float64)
    pos = np.einsum("nij,nj->ni", R, zz * np.exp(s)) + np.asarray(xyz, np.float32)[i].astype(np.float64)
    return pos, np.log(np.exp(s) / 1.6)


def densify_and_prune(scaling, opacity, accum, denom, **kw):
    """densify_and_prune's decisions and row map: classify()'s masks plus `cat_prune`, `src`, `slot` and `n_new`."""
    c = classify(scaling, opacity, accum, denom, **kw)
    c["cat_prune"] = cat_prune(c)
    c["src"], c["slot"] = _row_map([c["keep"], c["clone_kept"], c["children_kept"], c["children_kept"]])
    c["n_new"] = len(c["src"])
    return c


def prune_points(mask):
    """prune_points(mask): (src, slot) of the rows that stay, all originals."""
    return _row_map([~np.asarray(mask, bool).reshape(-1)])


def reset_opacity(opacity):
    """reset_opacity: inverse_sigmoid(min(sigmoid(o), 0.01)) = log(x / (1 - x)), in fp32."""
    x = np.minimum(_sigmoid32(opacity), RESET_CAP)
    return np.log(x / (np.float32(1.0) - x))


def _log_uniform(rs, lo, hi, n):
    return np.exp(rs.uniform(np.log(lo), np.log(hi), n))


def _scales(rs, lo, hi, n):
    """Log scales of n rows whose largest exp(s) lies in [lo, hi] (the other two components below it)."""
    top = _log_uniform(rs, lo, hi, n)
    s = np.log(top[:, None] * rs.uniform(0.2, 1.0, (n, 3)))
    s[np.arange(n), rs.integers(0, 3, n)] = np.log(top)
    return s.astype(np.float32)


def layout(n, kind, seed=0):
    """Category per row (KEEP ... CHILD_PRUNED).  kind "mixed": every category in every block of 1024.  kind "stretches"
    (blocks of 1024 rows, scan rounds of 256 blocks): mixed, then blocks 240..529 (a whole round) with no clone and no kept
    child, then blocks 760..1039 (a whole round) with every row pruned, then mixed again; clipped to n.  The last row is
    always a kept clone, so that a last block of a single row still puts rows into the map."""
    rs = np.random.default_rng(seed)
    cat = rs.choice(5, size=n, p=[0.4, 0.15, 0.15, 0.2, 0.1]).astype(np.int8)
    cat[-1:] = CLONE
    if kind == "stretches":
        a, b = 240 * 1024, 530 * 1024
        m = cat[a:b]
        cat[a:b] = np.where(rs.random(m.shape[0]) < 0.6, KEEP, np.where(rs.random(m.shape[0]) < 0.5, PRUNED, CHILD_PRUNED))
        a, b = 760 * 1024, 1040 * 1024
        m = cat[a:b]
        cat[a:b] = np.where(rs.random(m.shape[0]) < 0.6, PRUNED, CHILD_PRUNED)
    elif kind != "mixed":
        raise ValueError(kind)
    return cat


def synthetic_state(cat, seed=0, *, percent_dense=0.01, extent=1.0, grad_threshold=0.0002, min_opacity=0.05):
    """Deciding inputs whose rows fall in the given categories under both max_screen_size=None and a positive size, each
    input away from every threshold by far more than SCALE_MARGIN / OPACITY_MARGIN.  Returns fp32 arrays xyz [N,3],
    scaling [N,3], rotation [N,4], opacity [N,1], xyz_gradient_accum [N,1], denom [N,1], max_radii2D [N].

    KEEP: not selected, opaque, smax under 0.1 extent.  CLONE: selected, smax under percent_dense extent, opaque.  SPLIT:
    selected, smax over percent_dense extent, opaque, the children's smax under 0.1 extent (some sources above it).
    PRUNED: transparent, either unselected or selected as a clone.  CHILD_PRUNED: selected for a split, transparent."""
    cat = np.asarray(cat)
    n = cat.shape[0]
    rs = np.random.default_rng(seed + 1)
    split_at, world = percent_dense * extent, 0.1 * extent
    sel = (cat == CLONE) | (cat == SPLIT) | (cat == CHILD_PRUNED)
    pruned_clone = (cat == PRUNED) & (rs.random(n) < 0.5)
    sel |= pruned_clone
    small = (cat == CLONE) | ((cat == KEEP) & (rs.random(n) < 0.5)) | pruned_clone
    scaling = np.empty((n, 3), np.float32)
    scaling[small] = _scales(rs, 0.05 * split_at, 0.8 * split_at, int(small.sum()))
    big = ~small
    # big rows: smax in (1.25 percent_dense, 0.8 world), some split sources in (1.1 world, 1.5 world) whose children
    # (divided by 1.6) stay under 0.94 world
    hi = (cat == SPLIT) & big & (rs.random(n) < 0.3)
    lo = big & ~hi
    scaling[lo] = _scales(rs, 1.25 * split_at, 0.8 * world, int(lo.sum()))
    scaling[hi] = _scales(rs, 1.1 * world, 1.5 * world, int(hi.sum()))
    opaque = (cat == KEEP) | (cat == CLONE) | (cat == SPLIT)
    logit = lambda p: np.log(p / (1 - p))
    opacity = np.where(opaque, rs.uniform(logit(2.0 * min_opacity), 4.0, n),
                       rs.uniform(-9.0, logit(0.5 * min_opacity), n)).astype(np.float32)[:, None]
    denom = rs.integers(1, 30, n).astype(np.float32)
    g = np.where(sel, _log_uniform(rs, 1.5 * grad_threshold, 100 * grad_threshold, n),
                 _log_uniform(rs, 1e-4 * grad_threshold, 0.6 * grad_threshold, n))
    accum = (g * denom).astype(np.float32)
    # 0 / 0 (NaN -> 0, not selected) and x / 0 (inf, selected) on some rows
    zero = (rs.random(n) < 0.02)
    denom[zero] = 0.0
    accum[zero & ~sel] = 0.0
    accum[zero & sel] = np.float32(1e-3)
    xyz = rs.normal(size=(n, 3)).astype(np.float32)
    rotation = rs.normal(size=(n, 4)).astype(np.float32)
    rotation[np.abs(rotation).sum(1) < 0.1, 0] = 1.0
    max_radii2D = rs.uniform(50, 2000, n).astype(np.float32)  # would prune every row if it were read
    return dict(xyz=xyz, scaling=scaling, rotation=rotation, opacity=opacity, xyz_gradient_accum=accum[:, None],
                denom=denom[:, None], max_radii2D=max_radii2D)


def check_margins(state, *, percent_dense=0.01, extent=1.0, grad_threshold=0.0002, min_opacity=0.05):
    """True when no input lies within SCALE_MARGIN (sizes, gradients) or OPACITY_MARGIN (opacity) of a threshold,
    measured in float64."""
    s = np.exp(state["scaling"].astype(np.float64))
    smax, cmax = s.max(1), (s / 1.6).max(1)
    rel = lambda a, b: np.abs(a / b - 1.0).min() if a.size else np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        g = state["xyz_gradient_accum"].astype(np.float64).reshape(-1) / state["denom"].astype(np.float64).reshape(-1)
    g = g[np.isfinite(g)]
    op = 1.0 / (1.0 + np.exp(-state["opacity"].astype(np.float64).reshape(-1)))
    return (rel(smax, percent_dense * extent) > SCALE_MARGIN and rel(smax, 0.1 * extent) > SCALE_MARGIN and
            rel(cmax, 0.1 * extent) > SCALE_MARGIN and rel(g, grad_threshold) > SCALE_MARGIN and
            rel(op, min_opacity) > OPACITY_MARGIN)
