"""A restatement of csrc/texture.hip's spec (the input of the ColorMLP texture), written from the spec in float64 numpy,
forward and backward.  The spherical-harmonics bases are kept as polynomials -- lists of (coefficient, (i, j, k)) for
x^i y^j z^k -- with their constants from the closed forms, so values and derivatives both follow mechanically.
tests/test_texture_host.py pins it to the reference's own fp64 autograd results (tests/golden/texture.npz); the GPU tests
compare the kernels with it at the sizes the fixture does not cover."""
import numpy as np

PI = np.pi
C1 = np.sqrt(3 / (4 * PI))
C2 = np.sqrt(15 / (4 * PI)) * np.array([1, -1, 1 / (2 * np.sqrt(3)), -1, 0.5])
C3 = np.array([-np.sqrt(35 / (32 * PI)), np.sqrt(105 / (4 * PI)), -np.sqrt(21 / (32 * PI)), np.sqrt(7 / (16 * PI)),
               -np.sqrt(21 / (32 * PI)), np.sqrt(105 / (16 * PI)), -np.sqrt(35 / (32 * PI))])
C4 = np.array([0.75 * np.sqrt(35 / PI), -0.75 * np.sqrt(35 / (2 * PI)), 0.75 * np.sqrt(5 / PI), -0.75 * np.sqrt(5 / (2 * PI)),
               3 / 16 * np.sqrt(1 / PI), -0.75 * np.sqrt(5 / (2 * PI)), 3 / 8 * np.sqrt(5 / PI), -0.75 * np.sqrt(35 / (2 * PI)),
               3 / 16 * np.sqrt(35 / PI)])
X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _m(*vars_):
    return tuple(int(v) for v in np.sum(vars_, axis=0)) if vars_ else (0, 0, 0)


# basis k = 1..24 (the constant basis 0 is not part of the embedding): [(coefficient, exponents)]
BASES = [
    [(-C1, _m(Y))], [(C1, _m(Z))], [(-C1, _m(X))],
    [(C2[0], _m(X, Y))], [(C2[1], _m(Y, Z))], [(2 * C2[2], _m(Z, Z)), (-C2[2], _m(X, X)), (-C2[2], _m(Y, Y))],
    [(C2[3], _m(X, Z))], [(C2[4], _m(X, X)), (-C2[4], _m(Y, Y))],
    [(3 * C3[0], _m(X, X, Y)), (-C3[0], _m(Y, Y, Y))], [(C3[1], _m(X, Y, Z))],
    [(4 * C3[2], _m(Y, Z, Z)), (-C3[2], _m(X, X, Y)), (-C3[2], _m(Y, Y, Y))],
    [(2 * C3[3], _m(Z, Z, Z)), (-3 * C3[3], _m(X, X, Z)), (-3 * C3[3], _m(Y, Y, Z))],
    [(4 * C3[4], _m(X, Z, Z)), (-C3[4], _m(X, X, X)), (-C3[4], _m(X, Y, Y))],
    [(C3[5], _m(X, X, Z)), (-C3[5], _m(Y, Y, Z))], [(C3[6], _m(X, X, X)), (-3 * C3[6], _m(X, Y, Y))],
    [(C4[0], _m(X, X, X, Y)), (-C4[0], _m(X, Y, Y, Y))], [(3 * C4[1], _m(X, X, Y, Z)), (-C4[1], _m(Y, Y, Y, Z))],
    [(7 * C4[2], _m(X, Y, Z, Z)), (-C4[2], _m(X, Y))], [(7 * C4[3], _m(Y, Z, Z, Z)), (-3 * C4[3], _m(Y, Z))],
    [(35 * C4[4], _m(Z, Z, Z, Z)), (-30 * C4[4], _m(Z, Z)), (3 * C4[4], _m())],
    [(7 * C4[5], _m(X, Z, Z, Z)), (-3 * C4[5], _m(X, Z))],
    [(7 * C4[6], _m(X, X, Z, Z)), (-C4[6], _m(X, X)), (-7 * C4[6], _m(Y, Y, Z, Z)), (C4[6], _m(Y, Y))],
    [(C4[7], _m(X, X, X, Z)), (-3 * C4[7], _m(X, Y, Y, Z))],
    [(C4[8], _m(X, X, X, X)), (-6 * C4[8], _m(X, X, Y, Y)), (C4[8], _m(Y, Y, Y, Y))],
]
assert len(BASES) == 24

# the fixture's cases (tests/golden/make_texture_golden.py): name -> the module's settings and the camera's distance
CASES = {
    "deg1": dict(sh_degree=1, cano=1, use_xyz=0, latent_dim=16, train=0, dist=3.0, known_frame=1),
    "deg3": dict(sh_degree=3, cano=1, use_xyz=0, latent_dim=16, train=1, dist=0.3, known_frame=1),
    "deg4": dict(sh_degree=4, cano=1, use_xyz=0, latent_dim=16, train=1, dist=3.0, known_frame=1),
    "deg3_world": dict(sh_degree=3, cano=0, use_xyz=0, latent_dim=16, train=1, dist=3.0, known_frame=1),
    "deg3_xyz": dict(sh_degree=3, cano=1, use_xyz=1, latent_dim=16, train=1, dist=0.3, known_frame=1),
    "deg0_nolatent": dict(sh_degree=0, cano=1, use_xyz=0, latent_dim=0, train=1, dist=3.0, known_frame=1),
    "deg3_unknown_frame": dict(sh_degree=3, cano=1, use_xyz=0, latent_dim=16, train=0, dist=0.3, known_frame=0),
}
FEATURE_DIM, NON_RIGID_DIM, FRAMES = 32, 16, 5
INPUTS = ("features_dc", "features_rest", "xyz", "campos", "T_fwd", "noise", "non_rigid_feature", "latent_weight", "aabb", "g")
GRADS = ("d_features_dc", "d_features_rest", "d_xyz", "d_non_rigid_feature", "d_latent_weight")


def load_fixture(path):
    """tests/golden/texture.npz as a dict, with every "<name>_f64" rebuilt from "<name>_f32" + "<name>_f64res"."""
    d = np.load(path)
    out = {k: d[k] for k in d.files}
    for k in [k for k in out if k.endswith("_f64res")]:
        out[k[:-3]] = out[k[:-7] + "_f32"].astype(np.float64) + out.pop(k).astype(np.float64)
    return out


def n_sh(deg):
    return (deg + 1) ** 2 - 1


def _poly(terms, u, skip=None):
    """The polynomial's value at the rows of u (N, 3); with `skip` = an axis, its derivative along that axis."""
    out = np.zeros(u.shape[0])
    for c, e in terms:
        e = list(e)
        if skip is not None:
            if e[skip] == 0:
                continue
            c = c * e[skip]
            e[skip] -= 1
        out += c * u[:, 0] ** e[0] * u[:, 1] ** e[1] * u[:, 2] ** e[2]
    return out


def sh_embed(deg, u):
    """(N, (deg + 1)^2 - 1): the bases above the constant one at the rows of u."""
    return np.stack([_poly(t, u) for t in BASES[:n_sh(deg)]], axis=1) if deg > 0 else np.zeros((u.shape[0], 0))


def direction(xyz, campos, rot=None, noise=None):
    """(v, l, u): v = xyz - campos, rotated by R^T where `rot` (N, 3, 3) is given, times `noise` (3, 3) from the right
    where that is given; l = |v|; u = v / (l + 1e-12)."""
    v = xyz - campos.reshape(1, 3)
    if rot is not None:
        v = np.einsum("nba,nb->na", rot, v)
    if noise is not None:
        v = v @ noise
    l = np.sqrt((v * v).sum(1, keepdims=True))
    return v, l, v / (l + 1e-12)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _rot3(fwd_transform):
    return None if fwd_transform is None else _f64(fwd_transform)[:, :3, :3]


def _two_d(blocks, n):
    return [_f64(b).reshape(n, -1) for b in blocks]


def compose(before, xyz, campos, deg, fwd_transform=None, noise=None, after=(), latent=None):
    """inp (N, D) in float64: [before.. | sh_embed | after.. | latent]."""
    xyz = _f64(xyz)
    n = xyz.shape[0]
    cols = _two_d(before, n)
    if deg > 0:
        cols.append(sh_embed(deg, direction(xyz, _f64(campos), _rot3(fwd_transform), _f64(noise))[2]))
    cols += _two_d(after, n)
    if latent is not None and np.size(latent):
        cols.append(np.broadcast_to(_f64(latent).reshape(1, -1), (n, np.size(latent))))
    return np.concatenate(cols, axis=1)


def compose_backward(g, before, xyz, campos, deg, fwd_transform=None, noise=None, after=(), latent=None):
    """{"before": [..], "after": [..], "xyz", "latent"} in float64, each shaped as its input (latent: as given), for the
    upstream gradient g (N, D)."""
    xyz, g = _f64(xyz), _f64(g)
    n = xyz.shape[0]
    out, col = {"before": [], "after": []}, 0
    for b in before:
        w = int(np.prod(np.shape(b)[1:], dtype=np.int64))
        out["before"].append(g[:, col:col + w].reshape(np.shape(b)))
        col += w
    out["xyz"] = np.zeros((n, 3))
    if deg > 0:
        rot, noise = _rot3(fwd_transform), _f64(noise)
        v, l, u = direction(xyz, _f64(campos), rot, noise)
        gs = g[:, col:col + n_sh(deg)]
        du = np.stack([sum(gs[:, k] * _poly(BASES[k], u, skip=ax) for k in range(n_sh(deg))) for ax in range(3)], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            second = np.where(l > 0, v * (v * du).sum(1, keepdims=True) / (l * (l + 1e-12) ** 2), 0.0)
        dv = du / (l + 1e-12) - second
        if noise is not None:
            dv = dv @ noise.T
        if rot is not None:
            dv = np.einsum("nab,nb->na", rot, dv)
        out["xyz"] = dv
        col += n_sh(deg)
    for b in after:
        w = int(np.prod(np.shape(b)[1:], dtype=np.int64))
        out["after"].append(g[:, col:col + w].reshape(np.shape(b)))
        col += w
    if latent is not None and np.size(latent):
        out["latent"] = g[:, col:col + np.size(latent)].sum(0).reshape(np.shape(latent))
        col += np.size(latent)
    else:
        out["latent"] = None
    assert col == g.shape[1], (col, g.shape)
    return out


def case_call(fx, case):
    """The arguments of compose / compose_backward (and of color_mlp_input) for a fixture case, as a dict of numpy
    arrays, and the latent row's index."""
    c, p = CASES[case], case + "/"
    before = [fx[p + "features_dc"], fx[p + "features_rest"]]
    if c["use_xyz"]:
        lo, hi = fx[p + "aabb"].astype(np.float64)
        before.append(2 * (fx[p + "xyz"].astype(np.float64) - lo) / (hi - lo) - 1)
    row = int(fx[p + "latent_row"])
    kw = dict(before=before, xyz=fx[p + "xyz"], campos=fx[p + "campos"], deg=c["sh_degree"],
              fwd_transform=fx[p + "T_fwd"] if c["cano"] else None,
              noise=fx[p + "noise"] if (c["cano"] and c["train"]) else None, after=[fx[p + "non_rigid_feature"]],
              latent=fx[p + "latent_weight"][row] if c["latent_dim"] else None)
    return kw, row


def case_results(fx, case):
    """The restatement's results for a fixture case under the fixture's names ("inp" and GRADS)."""
    c, p = CASES[case], case + "/"
    kw, row = case_call(fx, case)
    got = {"inp": compose(**kw)}
    r = compose_backward(fx[p + "g"], **kw)
    got["d_features_dc"], got["d_features_rest"], got["d_non_rigid_feature"] = r["before"][0], r["before"][1], r["after"][0]
    got["d_xyz"] = r["xyz"]
    if c["use_xyz"]:  # xyz also enters through its normalised copy
        lo, hi = fx[p + "aabb"].astype(np.float64)
        got["d_xyz"] = got["d_xyz"] + r["before"][2] * 2 / (hi - lo)
    got["d_latent_weight"] = np.zeros(fx[p + "latent_weight"].shape)
    if c["latent_dim"]:
        got["d_latent_weight"][row] = r["latent"]
    return got


def random_inputs(n, widths_before, widths_after, lt, seed, dist=3.0, rot="4x4", noise=True):
    """Seeded fp32 inputs for n rows: points in [-1, 1]^3, the camera `dist` from the origin, rigid forward transforms."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = rng.normal(size=3)
    out = dict(before=[f32(rng.normal(size=(n, w))) for w in widths_before],
               after=[f32(rng.normal(size=(n, w))) for w in widths_after],
               xyz=f32(rng.uniform(-1, 1, size=(n, 3))), campos=f32(dist * d / np.linalg.norm(d)),
               latent=f32(rng.normal(size=lt)) if lt else None, fwd_transform=None, noise=None)
    if rot:
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        r, x, y, z = q.T
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                      1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                      1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
        if rot == "4x4":
            T = np.zeros((n, 4, 4))
            T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, rng.normal(scale=0.3, size=(n, 3)), 1.0
            out["fwd_transform"] = f32(T)
        else:
            out["fwd_transform"] = f32(R)
    if noise:
        a = rng.normal(scale=0.5, size=3)
        th = np.linalg.norm(a)
        k = a / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out["noise"] = f32(np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    return out
