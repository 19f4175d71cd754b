"""tests/golden/vi_ilr_update_hp.npz for the device-resident ILR VI tests (CPU and GPU): the inputs rebuilt as the entry points
take them, the 50-digit reference blocks, the per-block error metric, models built on exactly those priors, and the host
yardstick — each problem through the Python objects' own route (_update_from_stats(S, sample=False), canonical_expected(), the
three variational_lowerbound() terms), which is what meanfield_coordinate_descent_batched(resident=False) runs for an ILR model.
See tests/golden/make_vi_ilr_update_golden.py for what is stored and why the rest can be rebuilt exactly."""
import numpy as np

from conftest import load_golden
from mimo_amd.engine import SuffStats
from mimo_amd.utils.abstraction import Statistics as Stats
from mimo_amd.distributions import (CategoricalWithDirichlet, CategoricalWithStickBreaking, Dirichlet, TruncatedStickBreaking,
                                    StackedNormalWisharts, StackedGaussiansWithNormalWisharts, StackedMatrixNormalWisharts,
                                    StackedLinearGaussiansWithMatrixNormalWisharts)
from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians

# the blocks the error metric covers, under the names of BatchedHipEngine.vi_ilr_state
BLOCKS = ('g0', 'g1', 'e_log_pi',
          'qa', 'qb', 'qc', 'qd', 'mus', 'psis', 'nus', 'hld', 'cc', 'bb', 'W', 'E2', 'E4',
          'm_a', 'm_Kq', 'm_c', 'm_d', 'm_Ms', 'm_psis', 'm_nus', 'm_hld', 'm_Kinv', 'm_E1', 'm_E2', 'm_E4', 'm_cc',
          'c_total', 'j_bb', 'j_W', 'vlb')
GATINGS = ('dirichlet', 'stick-breaking')
_cache = {}


def _full(tri, n):
    """(B, K, n(n+1)/2) upper triangles -> (B, K, n, n) symmetric."""
    iu = np.triu_indices(n)
    out = np.zeros(tri.shape[:2] + (n, n))
    out[:, :, iu[0], iu[1]] = tri
    out[:, :, iu[1], iu[0]] = tri
    return out


def joint_stats(tables, rows):
    """Exact joint statistics of dyadic rows and weights (any summation order gives these float64 values)."""
    sn = np.stack([t.sum(axis=1) for t in tables])
    sz = np.stack([t @ z for t, z in zip(tables, rows)])
    szz = np.stack([np.einsum('kn,na,nb->kab', t, z, z) for t, z in zip(tables, rows)])
    return sn, sz, szz


def split(sn, sz, szz, dx):
    """split_joint_stats restated for arrays with leading axes (..., K): -> (S_yx~, S_x~x~, S_yy)."""
    syx = np.concatenate([szz[..., dx:, :dx], sz[..., dx:, None]], axis=-1)
    top = np.concatenate([szz[..., :dx, :dx], sz[..., :dx, None]], axis=-1)
    bot = np.concatenate([sz[..., None, :dx], sn[..., None, None]], axis=-1)
    return syx, np.concatenate([top, bot], axis=-2), szz[..., dx:, dx:]


def shapes():
    """-> one dict per shape of the fixture: B, dx, dy, K, gating, rows (list of (N_b, Dz)), tables (list of (K, N_b)), the exact
    statistics sn (B, K), sz (B, K, Dz), szz (B, K, Dz, Dz), the priors as vi_ilr_set_prior takes them (prior: gating, g0, g1,
    basis, experts) and in standard form (std), hp (the reference blocks) and vlb_scale (B, 3)."""
    if 'shapes' in _cache:
        return _cache['shapes']
    g = load_golden("vi_ilr_update_hp")
    out = []
    for idx, (B, dx, dy, K, stick) in enumerate(g["shapes"].tolist()):
        s = lambda name: g[f"s{idx}_{name}"]
        D, dc = dx + dy, dx + 1
        counts = s("rows").tolist()
        zo = to = 0
        rows, tables = [], []
        for n in counts:
            rows.append(s("Z")[zo:zo + n].astype(np.float64).reshape(n, D) / 8.0)
            tables.append(s("T")[to:to + K * n].astype(np.float64).reshape(K, n) / 16.0)
            zo, to = zo + n, to + K * n
        sn, sz, szz = joint_stats(tables, rows)
        # the natural parameters: float64 operations that are exact on these dyadic numbers (asserted by the generator)
        m0, kap, P0 = s("bm0"), s("bkappa0"), s("bpsi0inv")
        pa = kap[:, :, None] * m0
        pc = P0[:, None] + kap[:, :, None, None] * (m0[:, :, :, None] * m0[:, :, None, :])
        pd = np.full((B, K), 2.0)
        M0, K0, Y0 = s("M0"), s("K0"), s("ypsi0inv")
        ma = M0 @ K0[:, None]
        mb = np.ascontiguousarray(np.broadcast_to(K0[:, None], (B, K, dc, dc)))
        mc = Y0[:, None] + ma @ np.swapaxes(M0, 2, 3)
        md = np.full((B, K), 1.0 + dc)
        g0, g1 = s("g0"), s("g1")
        prior = dict(gating=GATINGS[stick], g0=g0, g1=g1 if stick else None, basis=(pa, kap.copy(), pc, pd, s("plz")),
                     experts=(ma, mb, mc, md, s("mlz")))
        std = dict(bm0=m0, bkappa0=kap, bpsi0inv=P0, M0=M0, K0=K0, ypsi0inv=Y0)
        hp = {name: s("hp_" + name) for name in ("mus", "hld", "cc", "bb", "E2", "E4", "m_Ms", "m_hld", "m_E1", "m_E4", "m_cc",
                                                 "e_log_pi", "c_total", "j_bb", "vlb")}
        hp["psis"], hp["W"] = _full(s("hp_psis_tri"), dx), _full(s("hp_W_tri"), dx)
        hp["m_psis"], hp["m_Kinv"], hp["m_E2"] = _full(s("hp_m_psis_tri"), dy), _full(s("hp_m_Kinv_tri"), dc), _full(s("hp_m_E2_tri"), dc)
        hp["j_W"] = _full(s("hp_j_W_tri"), D)
        # single float64 additions of exact numbers: the correctly rounded exact values
        syx, sxt, syy = split(sn, sz, szz, dx)
        if stick:
            acc = np.stack([np.array([np.sum(c[k + 1:]) for k in range(K)]) for c in sn])
            hp.update(g0=g0 + sn, g1=g1 + acc)
        else:
            hp.update(g0=((g0 - 1.0) + sn) + 1.0, g1=np.zeros((B, K)))
        hp.update(qa=pa + sz[:, :, :dx], qb=kap + sn, qc=pc + szz[:, :, :dx, :dx], qd=pd + sn, nus=pd + sn + dx,
                  m_a=ma + syx, m_Kq=mb + sxt, m_c=mc + syy, m_d=md + sn, m_nus=(md + sn) + dy + 1.0 - dc)
        out.append(dict(B=B, dx=dx, dy=dy, D=D, K=K, gating=GATINGS[stick], rows=rows, tables=tables, sn=sn, sz=sz, szz=szz,
                        prior=prior, std=std, hp=hp, vlb_scale=s("hp_vlb_scale")))
    _cache['shapes'] = out
    return out


def block_errors(state, shape):
    """name -> array of err = max|x - hp| / max|hp| per (problem, component) block ((B, K); the three terms of the bound, one
    block each per problem: (B, 3)).  A block that is reproduced exactly has err 0 whatever its size.  In the problem without
    rows the posterior is the prior and the three terms are exactly 0: for that problem alone |x - hp| is taken over the stored
    sum of the absolute values of the term's summands."""
    B, K = shape["B"], shape["K"]
    errs = {}
    for name in BLOCKS:
        x, hp = np.asarray(state[name], dtype=float), shape["hp"][name]
        assert x.shape == hp.shape, (name, x.shape, hp.shape)
        if name == 'vlb':
            diff = np.abs(x - hp)
            empty = np.array([len(z) == 0 for z in shape["rows"]])[:, None]
            with np.errstate(divide='ignore', invalid='ignore'):
                errs[name] = np.where(empty, diff / shape["vlb_scale"], np.where(diff == 0.0, 0.0, diff / np.abs(hp)))
            continue
        diff = np.abs(x - hp).reshape(B, K, -1).max(axis=2)
        size = np.abs(hp).reshape(B, K, -1).max(axis=2)
        with np.errstate(divide='ignore', invalid='ignore'):
            errs[name] = np.where(diff == 0.0, 0.0, diff / size)
    return errs


def build_model(K, dx, dy, gating, g0, g1, basis, experts, engine=None):
    """A BayesianMixtureOfLinearGaussians whose priors hold exactly these natural parameters and log-partitions (one problem's
    slices of what vi_ilr_set_prior takes): the standard parameters are derived, the natural ones are pinned in the priors' memo."""
    pa, pb, pc, pd, plz = (np.array(v, dtype=float) for v in basis)
    ma, mb, mc, md, mlz = (np.array(v, dtype=float) for v in experts)
    dc = dx + 1
    if gating == 'dirichlet':
        gate = CategoricalWithDirichlet(dim=K, prior=Dirichlet(dim=K, alphas=np.array(g0, dtype=float)))
    else:
        gate = CategoricalWithStickBreaking(dim=K, prior=TruncatedStickBreaking(dim=K, gammas=np.array(g0, dtype=float),
                                                                                deltas=np.array(g1, dtype=float)))
    bprior = StackedNormalWisharts(size=K, dim=dx)
    bprior.params = bprior.nat_to_std((pa, pb, pc, pd))
    bprior._set_memo(nat=Stats([pa, pb, pc, pd]), logZ=plz)
    mprior = StackedMatrixNormalWisharts(K, dc, dy)
    mprior.params = mprior.nat_to_std((ma, mb, mc, md))
    mprior._set_memo(nat=Stats([ma, mb, mc, md]), logZ=mlz)
    bs = StackedGaussiansWithNormalWisharts(size=K, dim=dx, prior=bprior, engine=engine)
    ms = StackedLinearGaussiansWithMatrixNormalWisharts(K, dc, dy, mprior, affine=True, engine=engine)
    return BayesianMixtureOfLinearGaussians(size=K, input_dim=dx, output_dim=dy, gating=gate, basis=bs, models=ms, engine=engine)


def model_of(shape, b, engine=None):
    pr = shape["prior"]
    return build_model(shape["K"], shape["dx"], shape["dy"], pr["gating"], pr["g0"][b], None if pr["g1"] is None else pr["g1"][b],
                       tuple(v[b] for v in pr["basis"]), tuple(v[b] for v in pr["experts"]), engine)


def model_blocks(model):
    """The blocks of a model's posteriors under the names of BatchedHipEngine.vi_ilr_state (m_bb and m_W included)."""
    K = model.size
    gp = model.gating.posterior
    o = {}
    if isinstance(gp, Dirichlet):
        o["g0"], o["g1"] = np.array(gp.alphas, dtype=float), np.zeros(K)
    else:
        o["g0"], o["g1"] = np.array(gp.gammas, dtype=float), np.array(gp.deltas, dtype=float)
    o["e_log_pi"] = np.asarray(model.gating.expected_log_gating(), dtype=float)
    bp = model.basis.posterior
    o["qa"], o["qb"], o["qc"], o["qd"] = (np.asarray(v, dtype=float) for v in bp.nat_param)
    o["mus"], _, o["psis"], o["nus"] = (np.asarray(v, dtype=float) for v in bp.params)
    o["hld"] = np.asarray(bp._half_logdet_psi(), dtype=float)
    o["cc"], o["bb"], o["W"] = (np.asarray(v, dtype=float) for v in bp.canonical_expected())
    E = bp.expected_statistics()
    o["E2"], o["E4"] = np.asarray(E[1], dtype=float), np.asarray(E[3], dtype=float)
    mp_ = model.models.posterior
    o["m_a"], o["m_Kq"], o["m_c"], o["m_d"] = (np.asarray(v, dtype=float) for v in mp_.nat_param)
    o["m_Ms"], Ks, o["m_psis"], o["m_nus"] = (np.asarray(v, dtype=float) for v in mp_.params)
    o["m_hld"] = np.asarray(mp_._half_logdet_psi(), dtype=float)
    o["m_Kinv"] = np.linalg.inv(Ks)
    E = mp_.expected_statistics()
    o["m_E1"], o["m_E2"], o["m_E4"] = (np.asarray(E[i], dtype=float) for i in (0, 1, 3))
    o["m_cc"], o["m_bb"], o["m_W"] = (np.asarray(v, dtype=float) for v in mp_.canonical_expected(affine=True))
    o["c_total"], o["j_bb"], o["j_W"] = (np.asarray(v, dtype=float) for v in model.canonical_expected())
    o["vlb"] = np.array([model.gating.variational_lowerbound(), np.sum(model.basis.variational_lowerbound()),
                         np.sum(model.models.variational_lowerbound())], dtype=float)
    return o


def host_update(model, sn, sz, szz):
    """One problem's update through the Python objects' own route -> its blocks."""
    model._update_from_stats(SuffStats(np.array(sn, dtype=float), np.array(sz, dtype=float), np.array(szz, dtype=float)),
                             sample=False)
    return model_blocks(model)


def host_state(shape):
    """The host yardstick on the fixture's inputs, with a leading problem axis."""
    per = [host_update(model_of(shape, b), shape["sn"][b], shape["sz"][b], shape["szz"][b]) for b in range(shape["B"])]
    return {name: np.stack([o[name] for o in per]) for name in per[0]}
