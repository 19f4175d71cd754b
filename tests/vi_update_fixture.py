"""tests/golden/vi_update_hp.npz for the device-resident VI tests (CPU and GPU): the inputs rebuilt as the entry points take them,
the 50-digit reference blocks, the per-block error metric and the host-native route on the same inputs.  See
tests/golden/make_vi_update_golden.py for what is stored and why the rest can be rebuilt exactly."""
import numpy as np

from conftest import load_golden
from mimo_amd import _lib

BLOCKS = ('alpha', 'qa', 'qb', 'qc', 'qd', 'mus', 'psis', 'nus', 'hld', 'cc', 'bb', 'W', 'E2', 'E4', 'e_log_pi', 'c_total', 'vlb')
_cache = {}


def _full(tri, D):
    """(B, K, D(D+1)/2) upper triangles -> (B, K, D, D) symmetric."""
    iu = np.triu_indices(D)
    out = np.zeros(tri.shape[:2] + (D, D))
    out[:, :, iu[0], iu[1]] = tri
    out[:, :, iu[1], iu[0]] = tri
    return out


def shapes():
    """-> one dict per shape of the fixture: B, D, K, rows (list of (N_b, D)), tables (list of (K, N_b)), the exact statistics
    sn (B, K), sx (B, K, D), sxx (B, K, D, D), the priors as vi_set_prior takes them, hp (the reference blocks under the names of
    BatchedHipEngine.vi_state) and vlb_scale (B, 2)."""
    if 'shapes' in _cache:
        return _cache['shapes']
    g = load_golden("vi_update_hp")
    out = []
    for idx, (B, D, K) in enumerate(g["shapes"].tolist()):
        s = lambda name: g[f"s{idx}_{name}"]
        counts = s("rows").tolist()
        zo = to = 0
        rows, tables = [], []
        for n in counts:
            rows.append(s("Z")[zo:zo + n].astype(np.float64).reshape(n, D) / 8.0)
            tables.append(s("T")[to:to + K * n].astype(np.float64).reshape(K, n) / 16.0)
            zo, to = zo + n, to + K * n
        # dyadic rows and weights: these float64 sums are exact whatever their order
        sn = np.stack([t.sum(axis=1) for t in tables])
        sx = np.stack([t @ z for t, z in zip(tables, rows)])
        sxx = np.stack([np.einsum('kn,na,nb->kab', t, z, z) for t, z in zip(tables, rows)])
        m0, kap, P0 = s("m0"), s("kappa0"), s("psi0inv")
        pa = kap[:, :, None] * m0
        pc = P0[:, None] + kap[:, :, None, None] * (m0[:, :, :, None] * m0[:, :, None, :])
        pd = np.full((B, K), 2.0)
        prior = dict(alpha0=s("alpha0"), pa=pa, pb=kap.copy(), pc=pc, pd=pd, prior_logZ=s("plz"))
        hp = {name: s("hp_" + name) for name in ("mus", "hld", "cc", "bb", "E2", "E4", "c_total", "vlb")}
        hp["e_log_pi"] = s("hp_elp")
        hp["psis"], hp["W"] = _full(s("hp_psis_tri"), D), _full(s("hp_W_tri"), D)
        # single float64 additions of exact numbers: the correctly rounded exact values (asserted by the generator)
        hp.update(alpha=prior["alpha0"] + sn, qa=pa + sx, qb=kap + sn, qc=pc + sxx, qd=pd + sn, nus=pd + sn + D)
        out.append(dict(B=B, D=D, K=K, rows=rows, tables=tables, sn=sn, sx=sx, sxx=sxx, prior=prior, hp=hp,
                        vlb_scale=s("hp_vlb_scale")))
    _cache['shapes'] = out
    return out


def block_errors(state, shape):
    """name -> array of err = max|x - hp| / max|hp| per (problem, component) block ((B, K); the two terms of the bound, one block
    each per problem: (B, 2)).  A block that is reproduced exactly has err 0 whatever its size.  One exception: in the problem
    without rows the posterior is the prior and both terms of the bound are exactly 0 (what the fixture holds there is the
    rounding of prior_logZ), so for that problem alone |x - hp| is taken over the stored sum of the absolute values of the
    term's summands."""
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


_SHAPES = lambda K, D: dict(alpha=(K,), qa=(K, D), qb=(K,), qc=(K, D, D), qd=(K,), mus=(K, D), psis=(K, D, D), nus=(K,), hld=(K,),
                            cc=(K,), bb=(K, D), W=(K, D, D), E2=(K,), E4=(K,), e_log_pi=(K,), c_total=(K,), vlb=(2,))


def host_sweep(K, D, prior, sn, sx, sxx):
    """One problem through the host-native route (mimo_host_gmm_vi_sweep + mimo_host_gmm_vi_bound, untied): prior = (alpha0,
    pa, pb, pc, pd, prior_logZ) of the problem -> its blocks under the names of BatchedHipEngine.vi_state, or None when a
    block is not positive definite."""
    lib = _lib.load()
    p = lambda a: a.ctypes.data
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    o = {name: np.zeros(s) for name, s in _SHAPES(K, D).items()}
    a0, pa, pb, pc, pd, plz = (c(v) for v in prior)
    sn, sx, sxx = c(sn), c(sx), c(sxx)
    rc = lib.mimo_host_gmm_vi_sweep(K, D, 0, p(a0), p(sn), p(pa), p(pb), p(pc), p(pd), p(sx), p(sn), p(sxx),
                                    p(o["alpha"]), p(o["qa"]), p(o["qb"]), p(o["qc"]), p(o["qd"]), p(o["mus"]), p(o["psis"]),
                                    p(o["nus"]), p(o["hld"]), None, p(o["cc"]), p(o["bb"]), p(o["W"]), p(o["E2"]), p(o["E4"]),
                                    p(o["e_log_pi"]), p(o["c_total"]))
    if rc != 0:
        return None
    rc = lib.mimo_host_gmm_vi_bound(K, D, 0, p(a0), p(o["alpha"]), p(o["e_log_pi"]), p(pa), p(pb), p(pc), p(pd), p(plz),
                                    p(o["qa"]), p(o["qb"]), p(o["qc"]), p(o["qd"]), p(o["mus"]), p(o["nus"]), p(o["hld"]), None,
                                    p(o["bb"]), p(o["E2"]), p(o["W"]), p(o["E4"]), p(o["vlb"]))
    assert rc == 0, rc
    return o


def host_state(shape):
    """The host-native route on the fixture's inputs, with a leading problem axis."""
    B, D, K = shape["B"], shape["D"], shape["K"]
    pr = shape["prior"]
    per = [host_sweep(K, D, tuple(pr[k][b] for k in ("alpha0", "pa", "pb", "pc", "pd", "prior_logZ")),
                      shape["sn"][b], shape["sx"][b], shape["sxx"][b]) for b in range(B)]
    return {name: np.stack([o[name] for o in per]) for name in _SHAPES(K, D)}
