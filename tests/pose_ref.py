"""Float64 numpy restatement of the fused SMPL pose correction (csrc/pose.hip carries the spec): the forward and the
analytic backward, written joint by joint in the order the kernels use.  tests/test_pose_host.py checks it against the
reference's own fp64 autograd results (tests/golden/pose.npz) to 1e-12; the GPU tests then compare the kernels with it
at shapes the fixture does not hold."""
import numpy as np

BONES = 24
SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int32)
LEFT, RIGHT = (1, 4, 7, 10), (2, 5, 8, 11)  # the leg chains of the A-pose -> star-pose transforms
OUTS = ("rots", "Jtrs", "bone_transforms", "loss_pose")
GRADS = ("dbetas", "droot_orient", "dpose_body", "dpose_hand", "dtrans")


def load_fixture(path):
    """tests/golden/pose.npz as a dict; `_f64res` arrays (float32 residuals from the fp32 result) become `_f64`."""
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    for k in [k for k in fx if k.endswith("_f64res")]:
        fx[k[:-3]] = fx[k[:-6] + "f32"].astype(np.float64) + fx[k].astype(np.float64)
    return fx


def synthetic_model(V, NB, seed, sign=0, parents=None):
    """A seeded body model of V vertices: a 1.7-unit cloud, small shape directions, a regressor with non-negative rows
    that sum to 1.  sign = +1 / -1 moves it so that every shaped coordinate is positive / negative for |betas| <= 3."""
    rng = np.random.default_rng(seed)
    v = rng.normal(scale=(0.3, 0.5, 0.15), size=(V, 3))
    sd = rng.normal(scale=0.01, size=(V, 3, NB))
    if sign:
        v += sign * (np.abs(v).max() + 3.0 * NB * np.abs(sd).max() + 0.25)
    k = min(V, 12)
    Jr = np.zeros((BONES, V))
    for j in range(BONES):
        idx = rng.choice(V, size=k, replace=False)
        Jr[j, idx] = rng.dirichlet(np.ones(k))
    return dict(v_template=v.astype(np.float32), shapedirs=sd.astype(np.float32), J_regressor=Jr.astype(np.float32),
                parents=(SMPL_PARENTS if parents is None else np.asarray(parents, np.int32)).copy())


def _skew(n):
    return np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])


def rodrigues(r):
    a = np.sqrt(((r + 1e-8) ** 2).sum())
    K = _skew(r / a)
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def rodrigues_backward(r, dR):
    a = np.sqrt(((r + 1e-8) ** 2).sum())
    n = r / a
    K = _skew(n)
    s, c = np.sin(a), np.cos(a)
    dK = s * dR + (1.0 - c) * (dR @ K.T + K.T @ dR)
    da = c * (dR * K).sum() + s * (dR * (K @ K)).sum()
    dn = np.array([dK[2, 1] - dK[1, 2], dK[0, 2] - dK[2, 0], dK[1, 0] - dK[0, 1]])
    da -= (dn * r).sum() / (a * a)
    return dn / a + da * (r + 1e-8) / a


def _star(j):
    """Q_j = the transpose of the fixed z rotation of joint j's 02v transform (+45 degrees on the left leg, -45 on the
    right, identity elsewhere) and the hip whose rest position its translation depends on (or -1)."""
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    if j in LEFT:
        return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]), LEFT[0]
    if j in RIGHT:
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), RIGHT[0]
    return np.eye(3), -1


def joints_linear(model):
    v, sd, Jr = (model[k].astype(np.float64) for k in ("v_template", "shapedirs", "J_regressor"))
    return Jr @ v, np.einsum("jv,vkl->jkl", Jr, sd)


def forward_backward(model, betas, root_orient, pose_body, pose_hand, trans, rots_gt=None, g_rots=None, g_Jtrs=None,
                     g_bone=None, g_loss=None):
    """All outputs (OUTS) and, for the given upstream gradients (None = zero), all gradients (GRADS), in float64."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    betas, root_orient, pose_body, pose_hand, trans = (f(a).reshape(-1) for a in (betas, root_orient, pose_body, pose_hand, trans))
    par = np.asarray(model["parents"]).astype(np.int64)
    Jt, Jsd = joints_linear(model)
    pose = np.concatenate([root_orient, pose_body, pose_hand]).reshape(BONES, 3)
    # rest joints and the statistics of the shaped template
    J = Jt + Jsd @ betas
    vs = model["v_template"].astype(np.float64) + model["shapedirs"].astype(np.float64) @ betas
    center = vs.mean(0)
    cmin, cmax = (vs - center).min(), (vs - center).max()
    pad = (cmax - cmin) * 0.05
    Jtrs = ((J - center - cmin + pad) / (cmax - cmin) / 1.1 - 0.5) * 2.0
    # the chain
    R = np.stack([rodrigues(pose[j]) for j in range(BONES)])
    Gr, Gt = np.zeros((BONES, 3, 3)), np.zeros((BONES, 3))
    Gr[0], Gt[0] = R[0], J[0]
    for i in range(1, BONES):
        p = par[i]
        Gr[i] = Gr[p] @ R[i]
        Gt[i] = Gr[p] @ (J[i] - J[p]) + Gt[p]
    # bone = A inv(B): A = [Gr | Gt - Gr J], B = [Q^T | (I - Q^T) J_hip]  =>  [Gr Q | Gt - Gr (J + (Q - I) J_hip) + trans]
    bone = np.zeros((BONES, 4, 4))
    bone[:, 3, 3] = 1.0
    u = np.zeros((BONES, 3))
    for i in range(BONES):
        Q, h = _star(i)
        u[i] = J[i] + ((Q - np.eye(3)) @ J[h] if h >= 0 else 0.0)
        bone[i, :3, :3] = Gr[i] @ Q
        bone[i, :3, 3] = Gt[i] - Gr[i] @ u[i] + trans
    rots = R.copy()
    rots[0] = np.eye(3)
    out = dict(rots=rots.reshape(1, BONES, 9), Jtrs=Jtrs.reshape(1, BONES, 3), bone_transforms=bone)
    if rots_gt is not None:
        diff = f(rots_gt).reshape(BONES, 3, 3) - rots
        out["loss_pose"] = (diff ** 2).mean()
    # ---- backward
    g_rots = np.zeros((BONES, 3, 3)) if g_rots is None else f(g_rots).reshape(BONES, 3, 3)
    g_bone = np.zeros((BONES, 4, 4)) if g_bone is None else f(g_bone).reshape(BONES, 4, 4)
    dJ = np.zeros((BONES, 3)) if g_Jtrs is None else f(g_Jtrs).reshape(BONES, 3) * (2.0 / (1.1 * (cmax - cmin)))
    dGr, dGt = np.zeros((BONES, 3, 3)), np.zeros((BONES, 3))
    dhip = np.zeros((BONES, 3))
    for i in range(BONES):
        Q, h = _star(i)
        gr, gt = g_bone[i, :3, :3], g_bone[i, :3, 3]
        dGr[i] = gr @ Q.T - np.outer(gt, u[i])
        dGt[i] = gt
        du = -Gr[i].T @ gt
        dJ[i] += du
        if h >= 0:
            dhip[i] = (Q - np.eye(3)).T @ du
    dtrans = g_bone[:, :3, 3].sum(0)
    for chain in (LEFT, RIGHT):
        for i in chain:
            dJ[chain[0]] += dhip[i]
    dR = np.zeros((BONES, 3, 3))
    for i in range(BONES - 1, 0, -1):
        p = par[i]
        dR[i] = Gr[p].T @ dGr[i]
        drel = Gr[p].T @ dGt[i]
        dJ[i] += drel
        dJ[p] -= drel
        dGr[p] += dGr[i] @ R[i].T + np.outer(dGt[i], J[i] - J[p])
        dGt[p] += dGt[i]
    dR[0] = dGr[0]
    dJ[0] += dGt[0]
    dRo = g_rots.copy()
    if rots_gt is not None and g_loss is not None:
        dRo += float(g_loss) * 2.0 * (rots - f(rots_gt).reshape(BONES, 3, 3)) / (BONES * 9)
    dRo[0] = 0.0  # rots[0] is the constant identity
    dpose = np.stack([rodrigues_backward(pose[j], dR[j] + dRo[j]) for j in range(BONES)]).reshape(-1)
    out.update(dbetas=np.einsum("jk,jkl->l", dJ, Jsd).reshape(1, -1), droot_orient=dpose[:3].reshape(1, 3),
               dpose_body=dpose[3:66].reshape(1, 63), dpose_hand=dpose[66:].reshape(1, 6), dtrans=dtrans.reshape(1, 3))
    return out


def torch_forward(model, betas, root_orient, pose_body, pose_hand, trans, rots_gt=None):
    """The same forward in plain torch, operator by operator and in the dtype of its inputs (gradients by autograd):
    the joints through the regressor, the chain as 4x4 products, the star-pose transforms accumulated along the leg
    chains and inverted numerically.  `model`: v_template (V, 3), shapedirs (V, 3, NB), J_regressor (24, V) tensors and
    `parents`.  Independent of the closed forms above: the end-to-end GPU test compares against it."""
    import torch
    v, sd, Jr = model["v_template"], model["shapedirs"], model["J_regressor"]
    par = [int(p) for p in model["parents"]]
    dt, dev = v.dtype, v.device
    vs = v + torch.einsum("l,vkl->vk", betas[0], sd)
    J = Jr @ vs
    r = torch.cat([root_orient, pose_body, pose_hand], dim=-1).reshape(BONES, 3)
    a = torch.sqrt(((r + 1e-8) ** 2).sum(1, keepdim=True))
    n = r / a
    z = torch.zeros_like(n[:, 0])
    K = torch.stack([z, -n[:, 2], n[:, 1], n[:, 2], z, -n[:, 0], -n[:, 1], n[:, 0], z], 1).reshape(BONES, 3, 3)
    R = torch.eye(3, dtype=dt, device=dev) + torch.sin(a)[..., None] * K + (1 - torch.cos(a))[..., None] * (K @ K)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dt, device=dev)

    def rigid(rot, t):
        return torch.cat([torch.cat([rot, t.reshape(3, 1)], 1), bottom], 0)

    G = [rigid(R[0], J[0])]
    for i in range(1, BONES):
        G.append(G[par[i]] @ rigid(R[i], J[i] - J[par[i]]))
    G = torch.stack(G)
    A = G.clone()
    A[:, :3, 3] = G[:, :3, 3] - torch.einsum("jrk,jk->jr", G[:, :3, :3], J)
    B = [torch.eye(4, dtype=dt, device=dev) for _ in range(BONES)]
    c = float(np.cos(np.pi / 4))
    for chain, s in ((LEFT, c), (RIGHT, -c)):
        Z = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=dt, device=dev)
        t = J[chain[0]]
        for k, j in enumerate(chain):
            if k > 0:
                t = Z @ (J[j] - J[chain[k - 1]]) + t
            B[j] = rigid(Z, t - Z @ J[j])
    bone = A @ torch.linalg.inv(torch.stack(B))
    bone = torch.cat([bone[:, :, :3], bone[:, :, 3:] + torch.cat([trans[0], torch.zeros(1, dtype=dt, device=dev)]).reshape(1, 4, 1)], 2)
    vd = vs.detach()
    center = vd.mean(0)
    cmax, cmin = (vd - center).max(), (vd - center).min()
    Jtrs = (((J - center) - cmin + (cmax - cmin) * 0.05) / (cmax - cmin) / 1.1 - 0.5) * 2.0
    rots = torch.cat([torch.eye(3, dtype=dt, device=dev)[None], R[1:]], 0).reshape(1, BONES, 9)
    loss = ((rots_gt.reshape(1, BONES, 9) - rots) ** 2).mean() if rots_gt is not None else None
    return rots, Jtrs.reshape(1, BONES, 3), bone, loss
