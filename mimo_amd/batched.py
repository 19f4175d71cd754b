"""BatchedHipEngine — one softmax pass over B independent problems (mimo_upload_batched / mimo_estep_batched).

B problems share Dz and K; each has its own rows and its own (c, b, W).  Where the reference fits many models with
joblib (examples/ilr/evaluate_sinc_parallel.py: one ILR fit per train split) or random restarts, every pass of every
fit is a chain of small launches; here one launch covers all of them.  A problem's results do not depend on what else
is in the batch, bit for bit.  No CPU fallback: without the library or a GPU the constructor raises.
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

    def estep(self, c, b, W, stats=True, keep_lse=False, entropy_split=False):
        """One pass over all problems.  c (B, K), b (B, K, Dz), W (B, K, Dz, Dz).  Returns (list of B SuffStats, or None
        without stats; scalars (B, 3)) — per problem what HipEngine.estep returns; scalars[:, 1:] are NaN unless
        entropy_split or keep_lse is set."""
        c, b, W, K = self._params(c, b, W)
        flags = ((0 if stats else _lib.F_NO_STATS) | (_lib.F_KEEP_LSE if keep_lse else 0)
                 | (_lib.F_ENTROPY_SPLIT if entropy_split else 0))
        D = self.D
        S = np.empty((self.B, K, 1 + D + D * D)) if stats else None
        sc = np.empty((self.B, 3))
        self._check(self._lib.mimo_estep_batched(self._ctx, _ptr(c), _ptr(b), _ptr(W), K, flags,
                                                 _ptr(S) if stats else None, _ptr(sc)))
        return ([SuffStats.from_packed(S[i], K, D) for i in range(self.B)] if stats else None), sc

    def get_lse(self):
        """Per-problem log-normalisers of the last pass with keep_lse: a list of B arrays (N_b,)."""
        out = np.empty(max(int(self.row_off[-1]), 1))
        self._check(self._lib.mimo_get_lse(self._ctx, _ptr(out)))
        return [out[self.row_off[i]:self.row_off[i + 1]].copy() for i in range(self.B)]
