"""BatchedHipEngine — one softmax pass, one Gibbs label pass or one table pass over B independent problems
(mimo_upload_batched / mimo_estep_batched / mimo_gibbs_labels_batched / mimo_label_stats_batched /
mimo_weighted_stats_batched / mimo_random_resp_stats_batched), or one softmax pass over chosen rows of every problem
(mimo_estep_batched_rows: the minibatch pass of batched SVI).

B problems share Dz and K; each has its own rows and its own (c, b, W).  Where the reference fits many models with
joblib (examples/ilr/evaluate_sinc_parallel.py: one ILR fit per train split) or random restarts, every pass of every
fit is a chain of small launches; here one launch covers all of them.  A problem's results do not depend on what else
is in the batch, bit for bit.  No CPU fallback: without the library or a GPU the constructor raises.

A nested batch (upload_shared) holds ONE data set that B problems read — the M inner mixtures of a mixture of mixtures
(mixtures/hgmm.py): estep(row_weights=...) is their weighted inner pass, outer_responsibilities the outer step, whose
(B, N) weights stay on the device for the next inner passes (mixtures/batched.py: meanfield_coordinate_descent_nested).
"""
import ctypes as C

import numpy as np

from . import _lib
from .engine import SuffStats, _f64, _ptr


class BatchedHipEngine:
    def __init__(self, device=0):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._lib.mimo_create(C.byref(self._ctx), int(device))
        if rc != 0:
            msg = self._lib.mimo_last_error(None).decode()
            self._ctx = None
            raise _lib.MimoHipError(f"mimo_create failed ({rc}): {msg}")
        self.device = int(device)
        self.B, self.D = 0, 0
        self.row_off = np.zeros(1, dtype=np.int64)
        self.shared = False           # upload_shared: the B problems read one block of rows

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.mimo_last_error(self._ctx).decode()
            raise _lib.MimoHipError(f"libmimo_hip error {rc}: {msg}")

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.mimo_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_structure(self, structure):
        """'full' (the only structure the batched pass covers), 'diag' or 'linear' (the pass then raises)."""
        self._check(self._lib.mimo_set_structure(self._ctx, {'full': 0, 'diag': 1, 'linear': 2}[structure]))

    def upload(self, arrays):
        """arrays: B host arrays of shape (N_b, Dz), copied once (concatenated on the device)."""
        arrays = [_f64(z) for z in arrays]
        if not arrays:
            raise ValueError("upload needs at least one problem")
        if any(z.ndim != 2 for z in arrays):
            raise ValueError("every problem's data must be (N_b, Dz)")
        D = arrays[0].shape[1]
        if any(z.shape[1] != D for z in arrays):
            raise ValueError(f"the problems' data dimensions differ: {[z.shape[1] for z in arrays]}")
        row_off = np.zeros(len(arrays) + 1, dtype=np.int64)
        row_off[1:] = np.cumsum([z.shape[0] for z in arrays])
        Z = np.ascontiguousarray(np.concatenate(arrays, axis=0)) if row_off[-1] > 0 else np.zeros((1, D))
        self._check(self._lib.mimo_upload_batched(self._ctx, _ptr(Z), _ptr(row_off), len(arrays), int(D)))
        self.B, self.D, self.row_off = len(arrays), int(D), row_off
        self.shared = False

    def upload_shared(self, Z, B):
        """ONE (N, Dz) host array that all B problems read (mimo_upload_batched_shared): copied once; the batch behaves as
        upload([Z] * B), bit for bit in every pass, with row_off = arange(B + 1) * N."""
        Z = _f64(Z)
        B = int(B)
        if Z.ndim != 2:
            raise ValueError("the shared data must be (N, Dz)")
        if Z.shape[0] < 1:
            raise ValueError("a shared batch needs at least one row")
        if B < 1:
            raise ValueError(f"a shared batch needs at least one problem, got B = {B}")
        N, D = Z.shape
        self._check(self._lib.mimo_upload_batched_shared(self._ctx, _ptr(Z), int(N), B, int(D)))
        self.B, self.D, self.row_off = B, int(D), np.arange(B + 1, dtype=np.int64) * int(N)
        self.shared = True

    def _stats_block(self, K):
        """The packed statistics block a pass fills: (B, K, 1 + Dz + Dz^2)."""
        return np.empty((self.B, K, 1 + self.D + self.D * self.D))

    def _stats_list(self, S, K):
        return [SuffStats.from_packed(S[i], K, self.D) for i in range(self.B)]

    def _per_problem(self, parts, count_msg, convert, each, dtype=np.float64, before=None):
        """A list of B per-problem arrays -> (the converted parts, their flattened concatenation as `dtype`: one zero for a
        batch without entries).  count_msg(n): the text when n != B parts came; convert: applied to every part;
        before(parts): the caller's checks across the converted parts; each(i, part, N_i): its checks of problem i's part
        against the problem's row count.  Raises ValueError before any library call."""
        parts = list(parts)
        if len(parts) != self.B:
            raise ValueError(count_msg(len(parts)))
        parts = [convert(p) for p in parts]
        if before is not None:
            before(parts)
        for i, p in enumerate(parts):
            each(i, p, int(self.row_off[i + 1] - self.row_off[i]))
        flat = np.concatenate([p.reshape(-1) for p in parts]) if sum(p.size for p in parts) else np.zeros(1, dtype=dtype)
        return parts, np.ascontiguousarray(flat, dtype=dtype)

    def _row_weights(self, row_weights):
        """A list of B arrays (N_b,), or one (B, N) array on a shared batch -> the concatenated weights; raises ValueError
        before any library call."""
        if isinstance(row_weights, np.ndarray) and row_weights.ndim == 2:
            if not getattr(self, 'shared', False):
                raise ValueError("one (B, N) weight array needs a shared batch (upload_shared); pass a list of B arrays")
            w = _f64(row_weights)
            if w.shape != (self.B, int(self.row_off[1])):
                raise ValueError(f"row_weights must be (B, N) = ({self.B}, {int(self.row_off[1])}), got shape {w.shape}")
            flat = w.reshape(-1)
        else:
            def each(i, p, n):
                if p.shape[0] != n:
                    raise ValueError(f"row_weights of problem {i} must hold one weight per datum ({n}), got {p.shape[0]}")
            _, flat = self._per_problem(row_weights, lambda n: f"row weights for {n} problems, {self.B} uploaded",
                                        lambda p: _f64(p).reshape(-1), each)
        if not np.all(np.isfinite(flat)) or np.any(flat < 0.):
            raise ValueError("row_weights must be finite and >= 0")
        return np.ascontiguousarray(flat)

    def _params(self, c, b, W):
        c, b, W = _f64(c), _f64(b), _f64(W)
        if c.ndim != 2:
            raise ValueError(f"c must be (B, K), got shape {c.shape}")
        B, K = c.shape
        if B != self.B:
            raise ValueError(f"parameters for {B} problems, {self.B} uploaded")
        if b.shape != (B, K, self.D) or W.shape != (B, K, self.D, self.D):
            raise ValueError(f"parameter shapes {c.shape}, {b.shape}, {W.shape} do not match B={B}, K={K}, Dz={self.D}")
        return c, b, W, K

    def _selection(self, rows):
        """B integer index arrays -> (the concatenated int64 indices, sel_off); raises ValueError before any library call."""
        def each(i, r, n):
            if r.ndim != 1:
                raise ValueError(f"the row selection of problem {i} must be one-dimensional, got shape {r.shape}")
            if r.dtype.kind not in 'iu':
                raise ValueError(f"the row selection of problem {i} must hold integers, got dtype {r.dtype}")
            if r.size and (int(r.min()) < 0 or int(r.max()) >= n):
                raise ValueError(f"the row selection of problem {i} holds an index outside [0, {n})")
        rows, flat = self._per_problem(rows, lambda n: f"row selections for {n} problems, {self.B} uploaded", np.asarray, each,
                                       dtype=np.int64)
        sel_off = np.zeros(self.B + 1, dtype=np.int64)
        sel_off[1:] = np.cumsum([r.size for r in rows])
        return flat, sel_off

    def estep(self, c, b, W, stats=True, keep_lse=False, entropy_split=False, rows=None, row_weights=None):
        """One pass over all problems.  c (B, K), b (B, K, Dz), W (B, K, Dz, Dz).  Returns (list of B SuffStats, or None
        without stats; scalars (B, 3)) — per problem what HipEngine.estep returns; scalars[:, 1:] are NaN unless
        entropy_split or keep_lse is set.
        rows: a list of B integer arrays, problem b's a selection of its local rows in [0, N_b) — any order, duplicates
        allowed, empty allowed.  The pass then runs over the selected rows only, gathered on the device from the resident
        batch (mimo_estep_batched_rows): per problem, bit for bit, what a plain pass returns on a batch that holds
        Z_b[rows_b].  No keep_lse with rows.
        row_weights: a list of B arrays (N_b,), one (B, N) array on a shared batch, or 'resident' (the weights of the last
        weighted pass or of outer_responsibilities, as they lie on the device): the statistics are those of r_kn * w_n, the
        scalars and a kept lse stay unweighted (mimo_estep_batched_weighted) — per problem what HipEngine.estep(row_weights=)
        returns.  Not together with rows."""
        w = None
        if row_weights is not None:
            if rows is not None:
                raise ValueError("row_weights together with rows: the minibatch pass takes no weights")
            if isinstance(row_weights, str):
                if row_weights != 'resident':
                    raise ValueError(f"row_weights must be arrays or 'resident', got {row_weights!r}")
            else:
                w = self._row_weights(row_weights)
        if rows is not None:
            if keep_lse:
                raise ValueError("keep_lse with rows: the normalisers of a selection have no place in the resident lse")
            sel, sel_off = self._selection(rows)
        c, b, W, K = self._params(c, b, W)
        flags = ((0 if stats else _lib.F_NO_STATS) | (_lib.F_KEEP_LSE if keep_lse else 0)
                 | (_lib.F_ENTROPY_SPLIT if entropy_split else 0))
        S = self._stats_block(K) if stats else None
        sc = np.empty((self.B, 3))
        if rows is not None:
            self._check(self._lib.mimo_estep_batched_rows(self._ctx, _ptr(c), _ptr(b), _ptr(W), K, _ptr(sel), _ptr(sel_off),
                                                          flags, _ptr(S) if stats else None, _ptr(sc)))
        elif row_weights is not None:
            self._check(self._lib.mimo_estep_batched_weighted(self._ctx, _ptr(c), _ptr(b), _ptr(W), K,
                                                              _ptr(w) if w is not None else None, flags,
                                                              _ptr(S) if stats else None, _ptr(sc)))
        else:
            self._check(self._lib.mimo_estep_batched(self._ctx, _ptr(c), _ptr(b), _ptr(W), K, flags,
                                                     _ptr(S) if stats else None, _ptr(sc)))
        return (self._stats_list(S, K) if stats else None), sc

    def _split(self, a):
        return [a[self.row_off[i]:self.row_off[i + 1]].copy() for i in range(self.B)]

    def gibbs_labels(self, c, b, W, seeds=None, sweep=0, u=None, stats=True, return_labels=True):
        """One label pass over all problems: per problem what HipEngine.gibbs_labels returns for its rows alone.
        seeds: B Philox keys (problem i draws with seed seeds[i], counter (local row, sweep)), or None with u; u: B arrays
        of uniforms, (N_b,) or (1, N_b) each.  Returns (list of B int32 arrays | None, list of B SuffStats | None)."""
        c, b, W, K = self._params(c, b, W)
        if u is not None:
            def each(i, ui, n):
                if ui.shape[0] != n:
                    raise ValueError("u must hold one uniform per datum")
            _, u = self._per_problem(u, lambda n: f"uniforms for {n} problems, {self.B} uploaded",
                                     lambda ui: _f64(ui).reshape(-1), each)
            sd = None
        else:
            if seeds is None:
                raise ValueError("gibbs_labels needs the uniforms u or one Philox seed per problem")
            sd = np.ascontiguousarray(np.asarray(seeds).reshape(-1).astype(np.uint64))
            if sd.shape[0] != self.B:
                raise ValueError(f"{sd.shape[0]} seeds for {self.B} problems")
        S = self._stats_block(K) if stats else None
        labels = np.empty(max(int(self.row_off[-1]), 1), dtype=np.int32) if return_labels else None
        self._check(self._lib.mimo_gibbs_labels_batched(
            self._ctx, _ptr(c), _ptr(b), _ptr(W), K, _ptr(sd) if sd is not None else None, int(sweep),
            _ptr(u) if u is not None else None, 0 if stats else _lib.F_NO_STATS,
            _ptr(labels) if return_labels else None, _ptr(S) if stats else None))
        return ((self._split(labels) if return_labels else None),
                (self._stats_list(S, K) if stats else None))

    def label_stats(self, labels, K):
        """Statistics of hard labels: a list of B int32 arrays (N_b,), or None for the labels of the last gibbs_labels.
        Returns a list of B SuffStats."""
        K = int(K)
        if labels is None:
            p = None
        else:
            def each(i, z, n):
                if z.shape[0] != n:
                    raise ValueError("labels must hold one entry per datum")
                if z.size and (z.min() < 0 or z.max() >= K):
                    raise ValueError("labels out of range")  # mirrors the assert in one_hot (data.py:162)
            _, labels = self._per_problem(labels, lambda n: f"labels for {n} problems, {self.B} uploaded",
                                          lambda z: np.asarray(z).reshape(-1), each, dtype=np.int32)
            p = _ptr(labels)
        S = self._stats_block(K)
        self._check(self._lib.mimo_label_stats_batched(self._ctx, p, K, 0, _ptr(S)))
        return self._stats_list(S, K)

    def _tables(self, tables):
        """B (K, N_b) weight tables -> (the concatenated K-major blocks, K); raises ValueError before any library call."""
        def before(tables):
            if not tables:
                raise ValueError("no batch is uploaded")
            if any(t.ndim != 2 for t in tables):
                raise ValueError("every problem's weights must be (K, N_b)")
            if any(t.shape[0] != tables[0].shape[0] for t in tables):
                raise ValueError(f"the problems' tables differ in K: {[t.shape[0] for t in tables]}")

        def each(i, t, n):
            if t.shape[1] != n:
                raise ValueError("weights must be (K, N_b): one column per datum")
        tables, flat = self._per_problem(tables, lambda n: f"tables for {n} problems, {self.B} uploaded", _f64, each, before=before)
        return flat, int(tables[0].shape[0])

    def weighted_stats(self, tables=None, K=None):
        """Statistics of arbitrary weights: a list of B arrays (K, N_b), one K for all problems (taken as they are), or
        None for the table the last random_resp_stats left on the device (K: its K).  Returns a list of B SuffStats —
        per problem what HipEngine.weighted_stats returns for its rows alone."""
        if tables is None:
            if K is None:
                raise ValueError("weighted_stats of the resident table needs its K")
            p, K = None, int(K)
        else:
            flat, K = self._tables(tables)
            p = _ptr(flat)
        S = self._stats_block(K)
        self._check(self._lib.mimo_weighted_stats_batched(self._ctx, p, K, 0, _ptr(S)))
        return self._stats_list(S, K)

    def random_resp_stats(self, K, seeds):
        """Statistics of random initial responsibilities drawn on the device, all problems in one launch: per problem what
        HipEngine.random_resp_stats(K, seeds[i]) returns for its rows alone (the same table, bit for bit).  seeds: B Philox
        keys.  The table stays resident (get_resp, weighted_stats(None, K)).  Returns a list of B SuffStats."""
        K = int(K)
        sd = np.ascontiguousarray(np.asarray(seeds).reshape(-1).astype(np.uint64))
        if sd.shape[0] != self.B:
            raise ValueError(f"{sd.shape[0]} seeds for {self.B} problems")
        S = self._stats_block(K)
        self._check(self._lib.mimo_random_resp_stats_batched(self._ctx, K, _ptr(sd), 0, _ptr(S)))
        self._K = K
        return self._stats_list(S, K)

    @staticmethod
    def _rows_form(a, B, d, what):
        """One (N, d) array (shared form) or a list of B arrays (ragged form) -> (rows (N_in, d), row_off | None, counts)."""
        if isinstance(a, (list, tuple)):
            if len(a) != B:
                raise ValueError(f"{what}: rows for {len(a)} problems, parameters for {B}")
            parts = [_f64(p) for p in a]
            parts = [p.reshape(-1, d) if p.ndim == 1 and d == 1 else p for p in parts]
            for i, p in enumerate(parts):
                if p.ndim != 2 or p.shape[1] != d:
                    raise ValueError(f"{what} of problem {i} must be (N_b, {d}), got shape {p.shape}")
            counts = [p.shape[0] for p in parts]
            row_off = np.zeros(B + 1, dtype=np.int64)
            row_off[1:] = np.cumsum(counts)
            flat = np.ascontiguousarray(np.concatenate(parts, axis=0)) if row_off[-1] > 0 else np.zeros((1, d))
            return flat, row_off, counts
        p = _f64(a)
        if p.ndim == 1 and d == 1:
            p = p.reshape(-1, 1)
        if p.ndim != 2 or p.shape[1] != d:
            raise ValueError(f"{what} must be (N, {d}) or a list of {B} such arrays, got shape {p.shape}")
        return (p if p.shape[0] > 0 else np.zeros((1, d))), None, [p.shape[0]] * B

    @staticmethod
    def _transform_block(t, B, d, what):
        if t is None:
            return None
        t = _f64(t)
        if t.shape != (B, 2, d):
            raise ValueError(f"{what} must be (B, 2, {d}) = (shift, scale) per problem, got shape {t.shape}")
        if not np.all(np.isfinite(t[:, 1])) or np.any(t[:, 1] == 0.):
            raise ValueError(f"{what}: every scale must be finite and nonzero")
        return t

    def predict(self, x, c, b, W, M, Q, Cc, mode='average', y=None, P=None, ld=None, variance='full', x_transform=None,
                y_transform=None):
        """Posterior-predictive mixture moments of B models in one launch (mimo_predict_batched): per problem what
        HipEngine.predict returns on the uploaded rows (x_b - shift_b) / scale_b, bit for bit, whatever else is in the batch.
        x: one (N, dx) array every problem reads (shared form: uploaded once) or a list of B arrays (N_b, dx) (ragged form);
        y (for nlpd, with P and ld) takes the form of x.  c (B, K), b (B, K, dx), W (B, K, dx, dx), M (B, K, dy, dx + 1),
        Q (B, K, dx + 1, dx + 1), Cc / P (B, K, dy, dy), ld (B, K): affine experts only, dx, dy <= 8.
        x_transform (B, 2, dx) / y_transform (B, 2, dy): per problem (shift, scale), applied in the kernel; None: rows as they are.
        Returns a list of B tuples (mu (N_b, dy), covar (N_b, dy, dy) | (var, std), nlpd (N_b,) | None).
        The rows are an argument, not state: B comes from c, nothing uploaded is read and nothing resident changes."""
        c, b, W = _f64(c), _f64(b), _f64(W)
        if c.ndim != 2:
            raise ValueError(f"c must be (B, K), got shape {c.shape}")
        B, K = c.shape
        if B < 1 or K < 1:
            raise ValueError(f"c must hold at least one problem and one component, got shape {c.shape}")
        if b.ndim != 3 or b.shape[:2] != (B, K) or b.shape[2] < 1:
            raise ValueError(f"b must be (B, K, dx) = ({B}, {K}, dx), got shape {b.shape}")
        dx = b.shape[2]
        if W.shape != (B, K, dx, dx):
            raise ValueError(f"W must be ({B}, {K}, {dx}, {dx}), got shape {W.shape}")
        M, Q, Cc = _f64(M), _f64(Q), _f64(Cc)
        if M.ndim != 4 or M.shape[:2] != (B, K) or M.shape[2] < 1:
            raise ValueError(f"M must be (B, K, dy, dx + 1) = ({B}, {K}, dy, {dx + 1}), got shape {M.shape}")
        dy = M.shape[2]
        if M.shape[3] != dx + 1:
            raise ValueError(f"affine experts only: M must be ({B}, {K}, {dy}, dx + 1 = {dx + 1}), got shape {M.shape}")
        if Q.shape != (B, K, dx + 1, dx + 1) or Cc.shape != (B, K, dy, dy):
            raise ValueError(f"predictive blocks {Q.shape}, {Cc.shape} do not match B={B}, K={K}, dy={dy}, dc={dx + 1}")
        if mode not in ('average', 'mode'):
            raise ValueError(f"mode must be 'average' or 'mode', got {mode!r}")
        if variance not in ('full', 'diagonal'):
            raise ValueError(f"variance must be 'full' or 'diagonal', got {variance!r}")
        X, row_off, counts = self._rows_form(x, B, dx, "x")
        xt = self._transform_block(x_transform, B, dx, "x_transform")
        yt = self._transform_block(y_transform, B, dy, "y_transform")
        Y = None
        if y is not None:
            if isinstance(y, (list, tuple)) != isinstance(x, (list, tuple)):
                raise ValueError("x and y must take the same form: both one array (shared) or both lists of B arrays (ragged)")
            if P is None or ld is None:
                raise ValueError("nlpd (y given) needs P (B, K, dy, dy) and ld (B, K)")
            P, ld = _f64(P), _f64(ld)
            if P.shape != (B, K, dy, dy) or ld.shape != (B, K):
                raise ValueError(f"nlpd needs P ({B}, {K}, {dy}, {dy}) and ld ({B}, {K}), got {P.shape}, {ld.shape}")
            Y, _, ycounts = self._rows_form(y, B, dy, "y")
            if ycounts != counts:
                raise ValueError(f"y must hold one row per row of x: {ycounts} against {counts}")
        elif yt is not None:
            raise ValueError("y_transform without y")
        diag = variance == 'diagonal'
        ncov = 2 * dy if diag else dy * dy
        total = int(sum(counts))
        mu = np.empty(max(total, 1) * dy)
        second = np.empty(max(total, 1) * ncov)
        nlpd = np.empty(max(total, 1)) if Y is not None else None
        self._check(self._lib.mimo_predict_batched(
            self._ctx, B, _ptr(X), _ptr(row_off) if row_off is not None else None, 0 if row_off is not None else counts[0], dx,
            _ptr(xt) if xt is not None else None, _ptr(c), _ptr(b), _ptr(W), K, _ptr(M), _ptr(Q), _ptr(Cc), dy,
            0 if mode == 'average' else 1, _ptr(Y) if Y is not None else None, _ptr(yt) if yt is not None else None,
            _ptr(P) if Y is not None else None, _ptr(ld) if Y is not None else None, _ptr(mu), _ptr(second),
            _ptr(nlpd) if Y is not None else None, _lib.F_DIAG_VAR if diag else 0))
        out, o = [], 0
        for n in counts:
            blk = second[o * ncov:(o + n) * ncov]
            if diag:
                sec = (blk[:n * dy].reshape(n, dy).copy(), blk[n * dy:].reshape(n, dy).copy())
            else:
                sec = blk.reshape(n, dy, dy).copy()
            out.append((mu[o * dy:(o + n) * dy].reshape(n, dy).copy(), sec, nlpd[o:o + n].copy() if Y is not None else None))
            o += n
        return out

    def outer_responsibilities(self, log_gating):
        """The outer step of a mixture of mixtures on a shared batch whose last pass kept its lse (mimo_outer_resp_batched):
        w[b, n] = softmax_b(lse[b, n] + log_gating[b]) stays on the device as the resident row weights
        (estep(row_weights='resident'), get_row_weights()).  Returns (counts (B,) = sum_n w[b, n], the outer
        log-likelihood sum_n logsumexp_b(lse[b, n] + log_gating[b]))."""
        lg = _f64(log_gating).reshape(-1)
        if lg.shape[0] != self.B:
            raise ValueError(f"log_gating has {lg.shape[0]} entries, {self.B} problems uploaded")
        if np.any(np.isnan(lg)) or np.any(lg == np.inf) or not np.any(np.isfinite(lg)):
            raise ValueError("log_gating must hold no NaN and no +inf, and one finite entry at least")
        out = np.empty(self.B + 1)
        self._check(self._lib.mimo_outer_resp_batched(self._ctx, _ptr(lg), 0, _ptr(out)))
        return out[:self.B].copy(), float(out[self.B])

    # ---- device-resident VI (mimo_vi_prior_batched / mimo_vi_run_batched / mimo_vi_get_batched) ----
    VI_PARTS = ('alpha', 'qa', 'qb', 'qc', 'qd', 'mus', 'psis', 'nus', 'hld', 'cc', 'bb', 'W', 'E2', 'E4', 'e_log_pi', 'c_total',
                'vlb')

    def _vi_part_shapes(self, K):
        D = self.D
        v, m = (K, D), (K, D, D)
        return ((K,), v, (K,), m, (K,), v, m, (K,), (K,), (K,), v, m, (K,), (K,), (K,), (K,), (2,))

    def vi_set_prior(self, alpha0, pa, pb, pc, pd, prior_logZ):
        """The priors of the B problems' mixtures of Gaussians (Dirichlet gating, untied Normal-Wishart components), copied to
        the device once: alpha0 (B, K), the Normal-Wishart natural parameters pa (B, K, Dz), pb (B, K), pc (B, K, Dz, Dz),
        pd (B, K) and their log-partitions prior_logZ (B, K), all finite.  Resets the loop: every problem active, its trace
        empty, its status clear.  An upload drops the priors."""
        alpha0, pa, pb, pc, pd, plz = (_f64(v) for v in (alpha0, pa, pb, pc, pd, prior_logZ))
        if alpha0.ndim != 2:
            raise ValueError(f"alpha0 must be (B, K), got shape {alpha0.shape}")
        B, K = alpha0.shape
        if B != self.B:
            raise ValueError(f"priors for {B} problems, {self.B} uploaded")
        D = self.D
        want = ((B, K), (B, K, D), (B, K), (B, K, D, D), (B, K), (B, K))
        got = tuple(v.shape for v in (alpha0, pa, pb, pc, pd, plz))
        if got != want:
            raise ValueError(f"prior shapes {got} do not match B={B}, K={K}, Dz={D}: {want}")
        if not all(np.all(np.isfinite(v)) for v in (alpha0, pa, pb, pc, pd, plz)):
            raise ValueError("the priors must be finite")
        self._check(self._lib.mimo_vi_prior_batched(self._ctx, K, _ptr(alpha0), _ptr(pa), _ptr(pb), _ptr(pc), _ptr(pd), _ptr(plz)))

    def _vi_run(self, call, K, iters, tol):
        K, iters, tol = int(K), int(iters), float(tol)
        if K < 1 or iters < 1:
            raise ValueError(f"K = {K} and iters = {iters} must be >= 1")
        if not tol >= 0.:
            raise ValueError(f"tol = {tol} must be >= 0")
        trace = np.empty((iters, self.B))
        n_done = np.empty(self.B, dtype=np.int32)
        status = np.empty(self.B, dtype=np.int32)
        self._check(getattr(self._lib, call)(self._ctx, K, iters, tol, 0, _ptr(trace), _ptr(n_done), _ptr(status)))
        return trace, n_done, status

    def _vi_unpack(self, call, K, names, shapes):
        """Every problem's current posterior block, split into its parts with a leading problem axis."""
        sizes = [int(np.prod(s)) for s in shapes]
        out = np.empty((self.B, sum(sizes)))
        self._check(getattr(self._lib, call)(self._ctx, K, _ptr(out)))
        state, o = {}, 0
        for name, shape, n in zip(names, shapes, sizes):
            state[name] = out[:, o:o + n].reshape((self.B,) + shape).copy()
            o += n
        return state

    def vi_run(self, K, iters, tol):
        """`iters` mean-field iterations of every problem that is still active, on the device: conjugate update from the
        statistics the last pass left resident, canonical form, batched pass, bound, stopping rule |vlb_t - vlb_{t-1}| < tol
        (mimo_vi_run_batched).  Returns (trace (iters, B), NaN where a problem appended nothing; n_done (B,), the bounds
        appended in this call; status (B,), bits: 1 for a problem one of whose blocks was not positive definite, 2 for one
        whose canonical form or bound was not finite — such a problem keeps the state of its last complete iteration).  The
        loop's passes are plain passes over all rows, whatever pass left the statistics it starts from.  The state persists
        across calls: vi_run(6) and vi_run(2) followed by vi_run(4) give the same bits."""
        return self._vi_run('mimo_vi_run_batched', K, iters, tol)

    def vi_state(self, K):
        """The posterior blocks the loop holds, as a dict of arrays with a leading problem axis: alpha, qa, qb, qc, qd (the
        natural parameters), mus, psis, nus, hld (standard parameters, half log det psi), cc, bb, W, E2, E4, e_log_pi,
        c_total (the canonical form of the next pass is (c_total, bb, W)), vlb (B, 2) = the Dirichlet term and the summed
        component terms of the bound — the parts of the host sweep (distributions/native_sweep.py)."""
        K = int(K)
        if K < 1:
            raise ValueError(f"K = {K} must be >= 1")
        return self._vi_unpack('mimo_vi_get_batched', K, self.VI_PARTS, self._vi_part_shapes(K))

    def _vi_resident(self, K):
        """Test hook: (the operand images the loop's passes read (B, ceil(K/16), F16/4, 64); the statistics the last pass left
        resident as a list of B SuffStats; its scalars (B, 3))."""
        K, D = int(K), self.D
        ns = ((D + 1) * (D + 2) // 2 + 15) // 16 * 4
        theta = np.empty((self.B, (K + 15) // 16, ns, 64))
        stats = np.empty(self.B * K * (1 + D + D * D) + 3 * self.B)
        self._check(self._lib.mimo_vi_get_theta_batched(self._ctx, K, _ptr(theta), _ptr(stats)))
        S = stats[:self.B * K * (1 + D + D * D)].reshape(self.B, K, 1 + D + D * D)
        return theta, self._stats_list(S, K), stats[S.size:].reshape(self.B, 3).copy()

    # ---- device-resident VI of mixtures of linear-Gaussian experts (mimo_vi_ilr_prior_batched / _run_ / _get_) ----
    # gating | basis (the GMM loop's names) | experts (m_*) | joint | bound
    VI_ILR_PARTS = ('g0', 'g1', 'e_log_pi',
                    'qa', 'qb', 'qc', 'qd', 'mus', 'psis', 'nus', 'hld', 'cc', 'bb', 'W', 'E2', 'E4',
                    'm_a', 'm_Kq', 'm_c', 'm_d', 'm_Ms', 'm_psis', 'm_nus', 'm_hld', 'm_Kinv', 'm_E1', 'm_E2', 'm_E4', 'm_cc',
                    'm_bb', 'm_W',
                    'c_total', 'j_bb', 'j_W', 'vlb')
    VI_GATINGS = {'dirichlet': 0, 'stick-breaking': 1}

    @staticmethod
    def _vi_ilr_part_shapes(K, dx, dy):
        dc, D = dx + 1, dx + dy
        s, x, xx = (K,), (K, dx), (K, dx, dx)
        return ((K,), (K,), (K,),
                x, s, xx, s, x, xx, s, s, s, x, xx, s, s,
                (K, dy, dc), (K, dc, dc), (K, dy, dy), s, (K, dy, dc), (K, dy, dy), s, s, (K, dc, dc), (K, dy, dc), (K, dc, dc), s, s,
                (K, D), (K, D, D),
                s, (K, D), (K, D, D), (3,))

    def vi_ilr_set_prior(self, gating, g0, g1, basis, experts):
        """The priors of the B problems' mixtures of linear-Gaussian experts over z = [x, y], copied to the device once.
        gating: 'dirichlet' (g0 (B, K) the concentrations, g1 None) or 'stick-breaking' (g0 the gammas, g1 the deltas, both
        (B, K)).  basis = (pa (B, K, dx), pb (B, K), pc (B, K, dx, dx), pd (B, K), log Z (B, K)): the Normal-Wishart natural
        parameters over x and their log-partitions.  experts = (ma (B, K, dy, dx + 1), mb (B, K, dx + 1, dx + 1),
        mc (B, K, dy, dy), md (B, K), log Z (B, K)): the matrix-normal-Wishart natural parameters of the affine experts.
        dx + dy must be the uploaded Dz; everything finite.  Resets the loop as vi_set_prior does (and replaces a GMM prior
        block: one family is resident at a time).  An upload drops the priors."""
        if gating not in self.VI_GATINGS:
            raise ValueError(f"gating = {gating!r} is not one of {sorted(self.VI_GATINGS)}")
        stick = gating == 'stick-breaking'
        if (g1 is None) == stick:
            raise ValueError("g1 (the deltas) goes with a stick-breaking gating and with that alone")
        if len(basis) != 5 or len(experts) != 5:
            raise ValueError("basis and experts are 5 arrays each: the four natural parameters and the log-partitions")
        g0 = _f64(g0)
        if g0.ndim != 2:
            raise ValueError(f"g0 must be (B, K), got shape {g0.shape}")
        B, K = g0.shape
        if B != self.B:
            raise ValueError(f"priors for {B} problems, {self.B} uploaded")
        g1 = _f64(g1) if stick else None
        pa, pb, pc, pd, plz = (_f64(v) for v in basis)
        ma, mb, mc, md, mlz = (_f64(v) for v in experts)
        if pa.ndim != 3 or ma.ndim != 4:
            raise ValueError(f"pa must be (B, K, dx) and ma (B, K, dy, dx + 1), got shapes {pa.shape} and {ma.shape}")
        dx, dy = pa.shape[2], ma.shape[2]
        if dx < 1 or dy < 1 or dx + dy != self.D:
            raise ValueError(f"dx = {dx} and dy = {dy} must be >= 1 and add up to the uploaded Dz = {self.D}")
        dc = dx + 1
        want = ((B, K),) * (2 if stick else 1) + ((B, K, dx), (B, K), (B, K, dx, dx), (B, K), (B, K),
                                                  (B, K, dy, dc), (B, K, dc, dc), (B, K, dy, dy), (B, K), (B, K))
        parts = ((g0, g1) if stick else (g0,)) + (pa, pb, pc, pd, plz, ma, mb, mc, md, mlz)
        got = tuple(v.shape for v in parts)
        if got != want:
            raise ValueError(f"prior shapes {got} do not match B={B}, K={K}, dx={dx}, dy={dy}: {want}")
        if not all(np.all(np.isfinite(v)) for v in parts):
            raise ValueError("the priors must be finite")
        self._check(self._lib.mimo_vi_ilr_prior_batched(
            self._ctx, K, dx, dy, self.VI_GATINGS[gating], _ptr(g0), _ptr(g1) if stick else None,
            _ptr(pa), _ptr(pb), _ptr(pc), _ptr(pd), _ptr(plz), _ptr(ma), _ptr(mb), _ptr(mc), _ptr(md), _ptr(mlz)))
        self._vi_ilr_dims = (dx, dy)

    def vi_ilr_run(self, K, iters, tol):
        """vi_run for the mixtures of linear-Gaussian experts whose priors vi_ilr_set_prior uploaded
        (mimo_vi_ilr_run_batched): the same returns, the same stopping rule, the same persistence across calls.  Status bit
        1: one of a component's three factorised blocks (the basis block, Kq, C) was not positive definite; bit 2: a joint
        canonical form or a term of the bound was not finite."""
        return self._vi_run('mimo_vi_ilr_run_batched', K, iters, tol)

    def vi_ilr_state(self, K):
        """The posterior blocks the ILR loop holds, as a dict of arrays with a leading problem axis (VI_ILR_PARTS):
        g0, g1 (alpha and zeros, or gammas and deltas), e_log_pi; the basis parts under the GMM loop's names (qa .. E4, over
        x); the experts' m_a, m_Kq, m_c, m_d (natural parameters), m_Ms, m_psis, m_nus, m_hld, m_Kinv, m_E1, m_E2, m_E4 and
        their canonical form m_cc, m_bb, m_W over z; the joint c_total, j_bb, j_W (the next pass's canonical form); vlb
        (B, 3) = the gating term, the summed basis terms, the summed expert terms of the bound."""
        K = int(K)
        if K < 1:
            raise ValueError(f"K = {K} must be >= 1")
        dims = getattr(self, '_vi_ilr_dims', None)
        if dims is None:
            raise ValueError("no ILR prior block was set (vi_ilr_set_prior)")
        return self._vi_unpack('mimo_vi_ilr_get_batched', K, self.VI_ILR_PARTS, self._vi_ilr_part_shapes(K, *dims))

    # ---- device-resident SVI (mimo_svi_state_batched / mimo_svi_run_batched and their _ilr_ forms) ----
    def _svi_status(self, call, *args):
        status = np.empty(self.B, dtype=np.int32)
        self._check(getattr(self._lib, call)(self._ctx, *args, _ptr(status)))
        return status

    def svi_set_state(self, alpha, qa, qb, qc, qd):
        """The starting posterior of the B mixtures of Gaussians whose priors vi_set_prior uploaded, as natural parameters:
        alpha (B, K) the Dirichlet concentrations, qa (B, K, Dz), qb (B, K), qc (B, K, Dz, Dz), qd (B, K), all finite.  Resets
        the loop, then derives on the device what the first minibatch pass and the first bound need: standard parameters,
        canonical form, operand image, prior terms (mimo_svi_state_batched).  Returns status (B,), vi_run's bits."""
        alpha, qa, qb, qc, qd = (_f64(v) for v in (alpha, qa, qb, qc, qd))
        if alpha.ndim != 2:
            raise ValueError(f"alpha must be (B, K), got shape {alpha.shape}")
        B, K = alpha.shape
        if B != self.B:
            raise ValueError(f"a state for {B} problems, {self.B} uploaded")
        D = self.D
        want = ((B, K), (B, K, D), (B, K), (B, K, D, D), (B, K))
        got = tuple(v.shape for v in (alpha, qa, qb, qc, qd))
        if got != want:
            raise ValueError(f"state shapes {got} do not match B={B}, K={K}, Dz={D}: {want}")
        if not all(np.all(np.isfinite(v)) for v in (alpha, qa, qb, qc, qd)):
            raise ValueError("the state must be finite")
        return self._svi_status('mimo_svi_state_batched', K, _ptr(alpha), _ptr(qa), _ptr(qb), _ptr(qc), _ptr(qd))

    def svi_ilr_set_state(self, g0, g1, basis, experts):
        """svi_set_state for the mixtures of linear-Gaussian experts whose priors vi_ilr_set_prior uploaded: g0, g1 (B, K) the
        gating's concentrations and None, or its gammas and deltas; basis = (qa (B, K, dx), qb (B, K), qc (B, K, dx, dx),
        qd (B, K)); experts = (a (B, K, dy, dx + 1), Kq (B, K, dx + 1, dx + 1), c (B, K, dy, dy), d (B, K))
        (mimo_svi_ilr_state_batched).  Returns status (B,)."""
        dims = getattr(self, '_vi_ilr_dims', None)
        if dims is None:
            raise ValueError("no ILR prior block was set (vi_ilr_set_prior)")
        if len(basis) != 4 or len(experts) != 4:
            raise ValueError("basis and experts are 4 arrays each: the natural parameters")
        dx, dy = dims
        dc = dx + 1
        g0 = _f64(g0)
        if g0.ndim != 2:
            raise ValueError(f"g0 must be (B, K), got shape {g0.shape}")
        B, K = g0.shape
        if B != self.B:
            raise ValueError(f"a state for {B} problems, {self.B} uploaded")
        parts = (g0,) + ((_f64(g1),) if g1 is not None else ()) + tuple(_f64(v) for v in tuple(basis) + tuple(experts))
        want = ((B, K),) * (2 if g1 is not None else 1) + ((B, K, dx), (B, K), (B, K, dx, dx), (B, K),
                                                           (B, K, dy, dc), (B, K, dc, dc), (B, K, dy, dy), (B, K))
        got = tuple(v.shape for v in parts)
        if got != want:
            raise ValueError(f"state shapes {got} do not match B={B}, K={K}, dx={dx}, dy={dy}: {want}")
        if not all(np.all(np.isfinite(v)) for v in parts):
            raise ValueError("the state must be finite")
        rest = parts[2:] if g1 is not None else parts[1:]
        return self._svi_status('mimo_svi_ilr_state_batched', K, _ptr(g0), _ptr(parts[1]) if g1 is not None else None,
                                *(_ptr(v) for v in rest))

    def _svi_run(self, call, K, iters, step_size, scale, batch_sizes, rows, seeds, resident_start):
        K, iters, step_size = int(K), int(iters), float(step_size)
        if K < 1 or iters < 1:
            raise ValueError(f"K = {K} and iters = {iters} must be >= 1")
        if not 0. < step_size <= 1.:
            raise ValueError(f"step_size = {step_size} outside (0, 1]")
        scale = _f64(scale).reshape(-1)
        if scale.shape != (self.B,):
            raise ValueError(f"scale must hold one factor per problem ({self.B}), got {scale.size}")
        if not np.all(np.isfinite(scale) & (scale > 0.)):
            raise ValueError(f"every scale must be finite and > 0, got {scale}")
        sizes = np.asarray(batch_sizes)
        if sizes.shape != (self.B,) or sizes.dtype.kind not in 'iu' or np.any(sizes < 0):
            raise ValueError(f"batch_sizes must hold one count >= 0 per problem ({self.B}), got {batch_sizes!r}")
        sel_off = np.zeros(self.B + 1, dtype=np.int64)
        sel_off[1:] = np.cumsum(sizes)
        per, n_sel = int(sel_off[-1]), iters - (1 if resident_start else 0)
        nrows = np.diff(self.row_off)
        flat = sd = None
        if rows is not None:
            if seeds is not None:
                raise ValueError("rows and seeds: give the indices or the Philox seeds, not both")
            rows = list(rows)
            if len(rows) != n_sel:
                raise ValueError(f"{len(rows)} selections for {iters} iterations"
                                 + (" after a resident start" if resident_start else "") + f": {n_sel} are needed")
            flat = np.empty((max(n_sel, 1), max(per, 1)), dtype=np.int64)
            for t, sel in enumerate(rows):
                if isinstance(sel, np.ndarray) and sel.ndim == 1 and sel.size == per:
                    sel = np.split(sel, sel_off[1:-1])
                sel = [np.asarray(r) for r in sel]
                if len(sel) != self.B:
                    raise ValueError(f"selection {t} holds the rows of {len(sel)} problems, {self.B} uploaded")
                for i, r in enumerate(sel):
                    if r.shape != (int(sizes[i]),) or (r.size and r.dtype.kind not in 'iu'):
                        raise ValueError(f"selection {t} of problem {i} must be {int(sizes[i])} integers, got shape {r.shape}, "
                                         f"dtype {r.dtype}")
                    if r.size and (int(r.min()) < 0 or int(r.max()) >= int(nrows[i])):
                        raise ValueError(f"selection {t} of problem {i} holds an index outside [0, {int(nrows[i])})")
                    flat[t, sel_off[i]:sel_off[i + 1]] = r
        elif seeds is not None:
            sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
            if sd.shape != (self.B,):
                raise ValueError(f"seeds must hold one Philox seed per problem ({self.B}), got {sd.size}")
            if n_sel > 0 and np.any((sizes > 0) & (nrows < 1)):
                raise ValueError("a problem without rows cannot draw a minibatch")
        elif n_sel > 0 and per > 0:
            raise ValueError("rows and seeds are both None: give the indices or one Philox seed per problem")
        trace = np.empty((iters, self.B))
        n_done = np.empty(self.B, dtype=np.int32)
        status = np.empty(self.B, dtype=np.int32)
        self._check(getattr(self._lib, call)(
            self._ctx, K, iters, step_size, _ptr(scale), _ptr(flat) if flat is not None else None, _ptr(sel_off),
            _ptr(sd) if sd is not None else None, _lib.F_SVI_RESIDENT_START if resident_start else 0, _ptr(trace), _ptr(n_done),
            _ptr(status)))
        return trace, n_done, status

    def svi_run(self, K, iters, step_size, scale, batch_sizes, rows=None, seeds=None, resident_start=False):
        """`iters` SVI iterations of every problem on the device (mimo_svi_run_batched), from the state svi_set_state
        uploaded or the last call left: minibatch pass, natural-gradient step
        eta <- (1 - step_size) eta + step_size (eta_prior + S / scale_b), canonical form, pass over all rows, bound.
        scale (B,): batch size / N_b, finite and > 0 (above 1 only for device draws of more slots than rows).
        batch_sizes (B,): the slots of problem b's minibatch, the same in every iteration.  rows: one selection per
        iteration, each a list of B integer arrays (or their concatenation), problem b's holding batch_sizes[b] local rows in
        [0, N_b); or seeds (B,): the indices are drawn on the device, slot j of problem b at iteration t =
        min(int(philox_uniform(seeds[b], j, t) * N_b), N_b - 1), t counted from svi_set_state.
        resident_start: the call's first iteration steps on the statistics already resident and takes no selection (rows
        then holds iters - 1).  Returns (trace (iters, B), n_done (B,), status (B,)) as vi_run; there is no stopping rule."""
        return self._svi_run('mimo_svi_run_batched', K, iters, step_size, scale, batch_sizes, rows, seeds, resident_start)

    def svi_ilr_run(self, K, iters, step_size, scale, batch_sizes, rows=None, seeds=None, resident_start=False):
        """svi_run for the mixtures of linear-Gaussian experts of vi_ilr_set_prior / svi_ilr_set_state
        (mimo_svi_ilr_run_batched)."""
        return self._svi_run('mimo_svi_ilr_run_batched', K, iters, step_size, scale, batch_sizes, rows, seeds,
                             resident_start)

    def get_row_weights(self):
        """The resident row weights (the last weighted pass's, or those of outer_responsibilities): a list of B arrays (N_b,)."""
        out = np.empty(max(int(self.row_off[-1]), 1))
        self._check(self._lib.mimo_get_row_weights_batched(self._ctx, _ptr(out)))
        return self._split(out)

    def get_resp(self, K=None):
        """The table of the last random_resp_stats, resident on the device: a list of B arrays (K, N_b)."""
        K = int(K if K is not None else getattr(self, '_K', 0))
        if K < 1:
            raise ValueError("get_resp needs the K of the resident table")
        out = np.empty(max(K * int(self.row_off[-1]), 1))
        self._check(self._lib.mimo_get_resp(self._ctx, _ptr(out)))
        ro = self.row_off
        return [out[K * ro[i]:K * ro[i + 1]].reshape(K, int(ro[i + 1] - ro[i])).copy() for i in range(self.B)]

    def get_labels(self):
        """The labels of the last gibbs_labels, resident on the device: a list of B int32 arrays (N_b,)."""
        out = np.empty(max(int(self.row_off[-1]), 1), dtype=np.int32)
        self._check(self._lib.mimo_get_labels(self._ctx, _ptr(out)))
        return self._split(out)

    def get_lse(self):
        """Per-problem log-normalisers of the last pass with keep_lse: a list of B arrays (N_b,)."""
        out = np.empty(max(int(self.row_off[-1]), 1))
        self._check(self._lib.mimo_get_lse(self._ctx, _ptr(out)))
        return self._split(out)
