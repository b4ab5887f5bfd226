"""Smoothed estimates from a recorded filter run without gathering a path (ScanHistory, ParticleHistory).

The smoothing marginal p(x_t | y_{1:T}) of a particle filter is step t's STORED particles under their descendant weights: for
particle j of step t, the final weight of all last-step particles whose lineage passes through j.  ``kernels.lineage_weights``
(gjx_lineage_weights) computes them for every step from the ancestor table by a backward scatter-add of integer weights; the moments
and quantile kernels then run step by step on rows that are already in place."""
from __future__ import annotations

import torch


class LineageSmoothing:
    """the four methods both history records share.  A record supplies ``_ancestor_table()`` (i32[T-1][K]), ``logw`` (the last step's
    log-weights) and ``_smoothing_rows(t, name)`` -> (rows f32[dim][K] — a view —, the row of the weights they stand under)."""

    def _lineage(self, check: bool = True) -> dict:
        """the outputs of the one gjx_lineage_weights call of this record.  ``check``: read n_bad back (once) and raise if a link
        left the collection; the smoothed_* methods ask for that AFTER they have enqueued their own launches, so the host does not
        wait for the scatter in front of them (such a link is harmless on the device: it is never an index)."""
        from .. import kernels
        if getattr(self, "_lineage_out", None) is None:
            self._lineage_out, self._lineage_checked = kernels.lineage_weights(self._ancestor_table(), self.logw), False
        if check and not self._lineage_checked:
            n_bad = int(self._lineage_out["n_bad"].item())             # (the one read-back)
            if n_bad != 0:
                raise ValueError(f"smoothing_weights: {n_bad} ancestor links point outside the collection")
            self._lineage_checked = True
        return self._lineage_out

    def smoothing_weights(self) -> torch.Tensor:
        """f32[T][K]: w[t][j] is the final weight of the last-step particles that descend from particle j of step t (every row sums to
        1); computed once by one gjx_lineage_weights call and kept.  ValueError if an ancestor link points outside [0, K)."""
        return self._lineage()["w"]

    def survivors(self) -> torch.Tensor:
        """i32[T]: the particles of every step that still have a descendant in the last step — the path-degeneracy diagnostic"""
        return self._lineage()["survivors"]

    def _smoothing_logw(self) -> torch.Tensor:
        """log of the smoothing weights, f32[T][K], one torch.log over the whole table (a zero weight: -inf, that is dead); kept"""
        if getattr(self, "_lineage_logw", None) is None:
            self._lineage_logw = torch.log(self._lineage(check=False)["w"])
        return self._lineage_logw

    def _smoothed_moments(self, name, cov: bool) -> dict:
        from .. import kernels
        lw, want = self._smoothing_logw(), "cov" if cov else "var"
        m = kernels.weighted_moments_steps([self._smoothing_rows(t, name) for t in range(lw.shape[0])], lw, want)
        self._lineage()
        return {"mean": m["mean"], want: m[want], "ess": m["stats"][:, 3]}

    def _smoothed_pair_moments(self, name) -> dict:
        """the lag-one pair (x_t, x_{t-1}) of every surviving path, t = 1 .. T-1, in one gjx_weighted_cross_moments call per pair.
        x_t and x_{t-1} are the rows ``_smoothing_rows`` gives steps t and t-1 — the values ``paths`` gives a trajectory —, so the two
        marginals of entry t-1 are ``smoothed_moments`` at t and t-1.  The pair stands under the weights of x_t's rows; where x_{t-1}'s
        rows stand under the step before (an ordinary history: step t-1's own rows), they are read through that step's ancestors;
        where both stand under one step (resample-move: the moved carry in the child's INPUT rows, at the child's index), there is
        no index."""
        from .. import kernels
        lw = self._smoothing_logw()
        T, dev = int(lw.shape[0]), lw.device
        rows = [self._smoothing_rows(t, name) for t in range(T)]
        d = int(rows[0][0].shape[0])
        if T == 1:
            self._lineage()
            e = lambda *s: torch.empty((0,) + s, dtype=torch.float32, device=dev)
            return {"mean": e(d), "mean_prev": e(d), "cross": e(d, d), "ess": e()}
        anc = self._ancestor_table()
        steps = []
        for t in range(1, T):
            (ra, ta), (rb, tb) = rows[t], rows[t - 1]
            assert tb in (ta, ta - 1)
            steps.append((ra, rb, None if tb == ta else anc[tb], ta))
        m = kernels.weighted_cross_moments_steps(steps, lw)
        self._lineage()
        return {"mean": m["mean_a"], "mean_prev": m["mean_b"], "cross": m["cross"], "ess": m["stats"][:, 3]}

    def _smoothed_quantiles(self, name, q) -> torch.Tensor:
        from .. import kernels
        lw = self._smoothing_logw()
        out = []
        for t in range(lw.shape[0]):
            rows, tw = self._smoothing_rows(t, name)
            out.append(kernels.weighted_quantiles(rows, lw[tw], q)["q"])
        self._lineage()
        return torch.stack(out)
