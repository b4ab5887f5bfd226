"""Importance sampling / SMC drivers with the reference's class names (inference/smc.py, sp.py).

Host code here only does what the reference does at trace time: key splits, constraint merging,
choosing site modes.  Every per-particle operation is one launch of the HIP kernels:
  run_smc            -> gjx_run_program (propagate + reweight + fused LSE partials)   smc.py:298-315
  log-ML estimate    -> 4-float device result of the LSE finish                       smc.py:96-97
  sample_particle    -> gjx_categorical_pick (Gumbel-max argmax reduce) + column read smc.py:102-109
  ChangeTarget       -> gjx_run_program with every site constrained                   smc.py:370-396
"""
from __future__ import annotations

from typing import Any

import numpy as np

from ..core import ChoiceMap, Key, split
from ..gen import GenerativeFunction, Marginal, Trace


class Target:
    """Unnormalised posterior: generative function + args + constraint (sp.py:52-94)."""

    def __init__(self, p: GenerativeFunction, args: tuple, constraint: ChoiceMap):
        if isinstance(p, Marginal):
            raise TypeError("Target does not support Marginal generative functions.")  # sp.py:46-49
        if not isinstance(p, GenerativeFunction):
            raise TypeError("Target needs a generative function")
        self.p, self.args, self.constraint = p, tuple(args), constraint

    def importance(self, key: Key, constraint: ChoiceMap, K: int | None = None):
        merged = self.constraint.merge(constraint)
        return self.p.importance(key, merged, self.args, K)

    def filter_to_unconstrained(self, choice_map: ChoiceMap) -> ChoiceMap:
        return choice_map.filter(~self.constraint.get_selection())

    def __getitem__(self, addr):
        return self.constraint[addr]

    def same_as(self, other: "Target") -> bool:
        from ..gen import _args_key
        return self.p is other.p and _args_key(self.args) == _args_key(other.args) and self.constraint == other.constraint

    def _cache_key(self):
        """Content identity for trace caches (a proposal ``q(target)`` is traced once per distinct target)."""
        from ..gen import _IdKey, _args_key, _value_key
        items = []
        from ..core import Masked
        for addr, v in self.constraint._d.items():
            items.append((repr(addr), (_value_key(v.value), _value_key(v.flag)) if isinstance(v, Masked) else _value_key(v)))
        return ("Target", _IdKey(self.p), _args_key(self.args), tuple(items))


class Moments:
    """Posterior means and variances of every choice of a weighted collection, computed by ONE gjx_weighted_moments call over the whole
    ``choices`` matrix (the reference's users write ``jnp.average(x, weights=w)`` per address).  ``mean(addr)`` / ``variance(addr)``
    are views into the device results: 0-d for a scalar site, f32[dim] for a vector site, f32[T][...] for the stacked name of Scan
    sites ``("x", t)`` (what ``Trace.get_choices`` stacks under ``"x"``); a collection of trials adds a leading ``n_trials`` axis.
    A site constrained to one shared value reports that value and variance 0.  Discrete sites are stored as floats: the mean of a
    ``flip`` is its posterior probability.  The variance is the population form: sum w (x - mean)^2 / sum w."""

    def __init__(self, trace: Trace, stats, mean, var):
        self._trace, self.stats, self._mean, self._var = trace, stats, mean, var     # stats [..][4], mean / var [..][n_slots]

    @property
    def ess(self):
        """effective sample size of the weights (0-d, or f32[n_trials])"""
        return self.stats[..., 3]

    def _site(self, arr, s, shared_value: bool):
        import torch
        slot = self._trace.prog.slot_of[s.addr]
        if slot >= 0:
            v = arr[..., slot:slot + s.dim]
        else:
            sh = np.broadcast_to(np.asarray(self._trace.shared[s.addr], np.float32).ravel(), (s.dim,)).copy()
            v = torch.as_tensor(sh if shared_value else np.zeros_like(sh), device=arr.device).expand(*arr.shape[:-1], s.dim)
        return v[..., 0] if s.dim == 1 else v

    def _get(self, arr, addr, shared_value: bool):
        import torch
        from ..core import key_of
        sl = self._trace.prog.site_list
        k = addr if addr in sl else key_of(addr)
        if k in sl:
            return self._site(arr, sl[k], shared_value)
        steps = [s for s in sl.sites if isinstance(s.addr, tuple) and len(s.addr) == 2 and s.addr[0] == k and isinstance(s.addr[1], int)]
        if not steps:
            raise KeyError(addr)
        return torch.stack([self._site(arr, s, shared_value) for s in steps], dim=arr.dim() - 1)

    def mean(self, addr):
        return self._get(self._mean, addr, True)

    def variance(self, addr):
        return self._get(self._var, addr, False)


def _moments_of(trace: Trace, log_weights, n_segments: int = 1) -> Moments:
    from .. import kernels
    rows = trace.choices if trace.choices.shape[0] > 0 else log_weights.reshape(1, -1)    # (no per-particle slot: the stats alone)
    m = kernels.weighted_moments(rows, log_weights, "var", n_segments)
    return Moments(trace, m["stats"], m["mean"], m["var"])


def _estimate_sites(trace: Trace, addr, lead: int, of_rows, of_shared):
    """an estimate of every component of the site(s) ``addr`` names, addresses resolved exactly as ``Moments._get`` resolves them:
    ``of_rows(rows [n][K])`` -> tensor [lead axes][n][X] for per-particle rows (ONE call where the sites' slots are adjacent),
    ``of_shared(value)`` -> tensor [lead axes][X] for a component constrained to one shared value.  -> [lead axes][T?][dim?][X]"""
    import torch
    from ..core import key_of
    sl = trace.prog.site_list
    k = addr if addr in sl else key_of(addr)
    if k in sl:
        sites, stacked = [sl[k]], False
    else:
        sites = [s for s in sl.sites if isinstance(s.addr, tuple) and len(s.addr) == 2 and s.addr[0] == k and isinstance(s.addr[1], int)]
        stacked = True
        if not sites:
            raise KeyError(addr)
    slots = [trace.prog.slot_of[s.addr] for s in sites]
    live = [(a, s.dim) for a, s in zip(slots, sites) if a >= 0]
    block, a0 = None, 0
    if len(live) > 1 and max(a + d for a, d in live) - min(a for a, _ in live) == sum(d for _, d in live):
        a0 = min(a for a, _ in live)
        block = of_rows(trace.choices[a0:max(a + d for a, d in live)])
    outs = []
    for a, s in zip(slots, sites):
        if a >= 0:
            v = block[..., a - a0:a - a0 + s.dim, :] if block is not None else of_rows(trace.choices[a:a + s.dim])
        else:
            sh = np.broadcast_to(np.asarray(trace.shared[s.addr], np.float32).ravel(), (s.dim,))
            v = torch.stack([of_shared(x) for x in sh], dim=lead)
        outs.append(v[..., 0, :] if s.dim == 1 else v)
    return torch.stack(outs, dim=lead) if stacked else outs[0]


def _quantile_of(trace: Trace, log_weights, addr, q, n_segments: int = 1, lead: int = 0):
    import torch
    from .. import _abi as A
    from .. import kernels
    scalar = isinstance(q, (int, float))
    levels = [float(q)] if scalar else [float(v) for v in q]
    dev = log_weights.device

    def of_rows(rows):
        r = kernels.weighted_quantiles(rows, log_weights, levels, n_segments)["q"]
        return r[None] if lead and n_segments == 1 else r

    def of_shared(x):                                     # one shared value: every quantile is that value
        return torch.full((n_segments,) * lead + (len(levels),), float(x), dtype=torch.float32, device=dev)

    if not levels or len(levels) > A.QUANTILES_MAX_LEVELS or any(not (0.0 <= v <= 1.0) for v in levels):
        raise ValueError(f"quantile({addr!r}): 1 to {A.QUANTILES_MAX_LEVELS} levels in [0, 1], not {levels}")
    out = _estimate_sites(trace, addr, lead, of_rows, of_shared)
    return out[..., 0] if scalar else out


def _histogram_of(trace: Trace, log_weights, addr, bins: int, span, n_segments: int = 1, lead: int = 0):
    """-> (mass [lead axes][T?][dim?][bins + 2], edges f32[bins + 1])"""
    import torch
    from .. import kernels
    dev = log_weights.device
    lo, hi, nb = np.float32(span[0]), np.float32(span[1]), int(bins)
    edges = []

    def of_rows(rows):
        h = kernels.weighted_histogram(rows, log_weights, nb, (lo, hi), n_segments)
        edges.append(h["edges"])
        return h["mass"][None] if lead and n_segments == 1 else h["mass"]

    def of_shared(x):                                     # one shared value: all the weight in its entry (the library's bin formula)
        x = np.float32(x)
        if x < lo:
            e = 0
        elif not x < hi:
            e = nb + 1
        else:
            b = np.floor(np.float32(np.float32(x - lo) * (np.float32(nb) / np.float32(hi - lo))))
            e = 1 + int(b) if b < nb else nb + 1
        m = torch.zeros((n_segments,) * lead + (nb + 2,), dtype=torch.float32, device=dev)
        m[..., e] = 1.0
        return m

    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi) or nb <= 0:
        raise ValueError(f"histogram({addr!r}): bins > 0 and a finite range with lo < hi, not {bins}, {tuple(span)}")
    mass = _estimate_sites(trace, addr, lead, of_rows, of_shared)
    if not edges:
        edges.append(torch.tensor([float(lo) + (float(hi) - float(lo)) * i / nb for i in range(nb)] + [float(hi)], dtype=torch.float32, device=dev))
    return mass, edges[0]


def _probabilities_of(trace: Trace, log_weights, addr, n_segments: int = 1, lead: int = 0):
    """posterior probabilities of the values 0 .. ncat - 1 of a discrete site: the histogram with one bin per value, inner bins only"""
    from .. import _abi as A
    from ..core import key_of
    sl = trace.prog.site_list
    k = addr if addr in sl else key_of(addr)
    s = sl[k]
    ncat = 2 if s.kind in (A.FLIP, A.BERNOULLI_LOGITS) else int(s.ncat)
    if ncat <= 0:
        raise ValueError(f"probabilities({addr!r}): the site is neither a flip nor a categorical; use histogram(addr, bins, range)")
    mass, _ = _histogram_of(trace, log_weights, k, ncat, (-0.5, ncat - 0.5), n_segments, lead)
    return mass[..., 1:ncat + 1]


def pareto_k_threshold(K: int) -> float:
    """min(1 - 1 / log10(K), 0.7): the k-hat below which K importance draws give a reliable estimate (the sample-size-dependent
    threshold of the PSIS paper; 0.7 from K = 2200 up)"""
    import math
    return min(1.0 - 1.0 / math.log10(K), 0.7)


class ParticleCollection:
    """Weighted particles (smc.py:76-109): a batched Trace + log-weights, all on the device."""

    def __init__(self, particles: Trace, log_weights, is_valid=True, lse=None, offset: int = 0, K_total=None, partials=None):
        self.particles, self.log_weights, self.is_valid = particles, log_weights, is_valid
        self._lse = lse            # device f32[4] = {max, sumexp, lse, lse - log K} when already reduced
        self._partials = partials  # kernels.RunPartials of the producing run (block {max, sumexp} pairs), or None
        self.offset = offset
        self.K_total = K_total or int(log_weights.shape[0])

    def get_particles(self) -> Trace:
        return self.particles

    def get_particle(self, idx) -> Trace:
        return self.particles.get_particle(idx)

    def get_log_weights(self):
        return self.log_weights

    def __len__(self):
        return int(self.log_weights.shape[0])

    def __getitem__(self, idx):
        return self.get_particle(idx), self.log_weights[idx]

    def lse(self):
        """The LSE record, reduced on first use: from the producing run's block partials while they are still in its
        workspace (one small launch), otherwise from the log-weights."""
        if self._lse is None:
            from .. import kernels
            p = self._partials
            if p is not None and p.valid():
                self._lse = p.finish(self.K_total)
            else:
                self._lse = kernels.logsumexp(self.log_weights, self.K_total)
        return self._lse

    def effective_sample_size(self):
        """ESS = (sum w)^2 / sum w^2 of the collection's weights: a 0-d device tensor (gjx_ess, one launch; Gen's effective_sample_size)"""
        from .. import kernels
        return kernels.ess(self.log_weights)[3]

    def moments(self) -> Moments:
        """posterior mean and variance of every choice under the collection's weights (one gjx_weighted_moments call, kept)"""
        if getattr(self, "_moments", None) is None:
            self._moments = _moments_of(self.particles, self.log_weights)
        return self._moments

    def mean(self, addr):
        """E[addr] under the self-normalised weights: ``moments().mean(addr)``"""
        return self.moments().mean(addr)

    def variance(self, addr):
        """Var[addr] (population form) under the self-normalised weights: ``moments().variance(addr)``"""
        return self.moments().variance(addr)

    def covariance(self, addr):
        """f32[dim][dim]: the weighted covariance matrix of the components of ONE site, from one gjx_weighted_moments call over its rows"""
        import torch
        from .. import _abi as A
        from .. import kernels
        from ..core import key_of
        tr = self.particles
        sl = tr.prog.site_list
        s = sl[addr if addr in sl else key_of(addr)]
        if s.dim > A.MOMENTS_MAX_COV_ROWS:
            raise ValueError(f"covariance({addr!r}): the site has {s.dim} components, a covariance takes at most {A.MOMENTS_MAX_COV_ROWS}")
        slot = tr.prog.slot_of[s.addr]
        if slot < 0:                                      # one shared value: no spread
            return torch.zeros((s.dim, s.dim), dtype=torch.float32, device=self.log_weights.device)
        return kernels.weighted_moments(tr.choices[slot:slot + s.dim], self.log_weights, "cov")["cov"]

    def cross_covariance(self, addr_a, addr_b):
        """f32[dim_a][dim_b]: the weighted covariance between the components of TWO sites, sum w (a - E a)(b - E b)^T (population
        form), from one gjx_weighted_cross_moments call over their rows (no index: both sites of one particle).
        ``cross_covariance(a, a)`` is ``covariance(a)`` up to rounding.  A site constrained to one shared value has no spread: zeros.
        Trials (TrialCollections) and segments are out of scope: the call takes one collection."""
        import torch
        from .. import _abi as A
        from .. import kernels
        from ..core import key_of
        tr = self.particles
        sl = tr.prog.site_list
        keys = [addr if addr in sl else key_of(addr) for addr in (addr_a, addr_b)]
        for addr, k in zip((addr_a, addr_b), keys):
            if k not in sl:
                raise KeyError(addr)
        sa, sb = sl[keys[0]], sl[keys[1]]
        for addr, s in ((addr_a, sa), (addr_b, sb)):
            if s.dim > A.MOMENTS_MAX_COV_ROWS:
                raise ValueError(f"cross_covariance({addr!r}): the site has {s.dim} components, a side takes at most {A.MOMENTS_MAX_COV_ROWS}")
        slot_a, slot_b = tr.prog.slot_of[sa.addr], tr.prog.slot_of[sb.addr]
        if slot_a < 0 or slot_b < 0:                      # one shared value: no spread
            return torch.zeros((sa.dim, sb.dim), dtype=torch.float32, device=self.log_weights.device)
        return kernels.weighted_cross_moments(tr.choices[slot_a:slot_a + sa.dim], tr.choices[slot_b:slot_b + sb.dim], self.log_weights)["cross"]

    def quantile(self, addr, q):
        """the weighted quantile(s) of a site at the level(s) ``q`` in [0, 1] (NumPy's "inverted_cdf" under the self-normalised weights:
        always the value of a live particle; one gjx_weighted_quantiles call, a radix select — no sort): 0-d for a scalar site and a
        scalar ``q``, else [dim], [n_levels] or [dim][n_levels]; [T][...] for the stacked name of Scan sites.  A site constrained to one
        shared value reports that value."""
        return _quantile_of(self.particles, self.log_weights, addr, q)

    def median(self, addr):
        """``quantile(addr, 0.5)``"""
        return self.quantile(addr, 0.5)

    def credible_interval(self, addr, mass: float = 0.9):
        """the equal-tailed interval that holds ``mass`` of the posterior: the quantiles at (1 - mass) / 2 and (1 + mass) / 2 on a
        trailing axis of size 2"""
        m = float(mass)
        if not 0.0 <= m <= 1.0:
            raise ValueError(f"credible_interval({addr!r}): mass must be in [0, 1], not {mass}")
        return self.quantile(addr, ((1.0 - m) / 2.0, (1.0 + m) / 2.0))

    def histogram(self, addr, bins: int, range):
        """the weighted marginal of a site over ``bins`` equal bins of ``range`` = (lo, hi) (one gjx_weighted_histogram call)
        -> (mass [dim?][bins + 2], edges f32[bins + 1]); mass[..., 0] is the weight below lo, mass[..., bins + 1] the weight at or above
        hi (and of NaN values), and the entries of a row sum to 1"""
        return _histogram_of(self.particles, self.log_weights, addr, bins, range)

    def probabilities(self, addr):
        """the posterior probabilities of a discrete site: f32[2] for a flip, f32[ncat] for a categorical (ValueError for any other)"""
        return _probabilities_of(self.particles, self.log_weights, addr)

    def _pareto(self) -> dict:
        """ONE gjx_pareto_smooth call for pareto_k() and pareto_smoothed(), kept"""
        if getattr(self, "_psis", None) is None:
            from .. import kernels
            if self.K_total != len(self):
                raise NotImplementedError("Pareto smoothing of a shard of a larger collection: the tail is that of the whole collection")
            self._psis = kernels.pareto_smooth(self.log_weights)
        return self._psis

    def pareto_k(self):
        """the Pareto k-hat diagnostic of the weights: the shape of the generalised Pareto distribution fitted to the largest
        min(K / 5, 3 sqrt K) of them (gjx_pareto_smooth), a 0-d device tensor.  Below about 0.5 the estimates are reliable, above
        ``inference.pareto_k_threshold(K)`` (0.7 for large K) they are not, whatever the effective sample size says; NaN where there
        is no tail to fit (equal weights, fewer than 25 particles)."""
        return self._pareto()["k"]

    def pareto_smoothed(self) -> "ParticleCollection":
        """the same particles under Pareto-smoothed weights: the largest weights replaced by the quantiles of the fitted distribution
        (a small bias for a large cut in variance).  ``mean``, ``quantile``, ``effective_sample_size`` and the log-ML estimate of the
        result run on the smoothed weights."""
        return ParticleCollection(self.particles, self._pareto()["logw"], self.is_valid, None, self.offset, self.K_total)

    def lse_partials(self):
        """kernels.RunPartials of the producing run if still valid (for ``inference.pf.resample(..., collection=)``)"""
        p = self._partials
        return p if (self._lse is None and p is not None and p.valid()) else None

    def get_log_marginal_likelihood_estimate(self):
        """logsumexp(log_weights) - log K  (smc.py:96-97), a 0-d device tensor."""
        return self.lse()[3]

    def sample_particle(self, key: Key) -> Trace:
        """1-of-K categorical draw over the weights + gather (smc.py:102-109)."""
        from .. import kernels
        out = kernels.categorical_pick(self.log_weights, self.lse(), key, self.particles.prog.rng_mode, self.offset)
        idx = int(out[1].item()) - self.offset
        return self.get_particle(idx)


class TrialCollections:
    """n independent particle collections of K particles each, produced by ONE launch over n K particles: what the reference
    gets from ``jax.vmap(alg.run_smc)(jax.random.split(key, n))`` (README.md:108-113).  Trial t owns the global particle
    indices [t K, (t + 1) K); its weights are those of ``alg.run_smc(key, offset=t K, K_local=K)`` of an n K-particle run,
    normalised on their own."""

    def __init__(self, particles: Trace, log_weights, n_trials: int, K: int):
        self.particles, self.log_weights, self.n_trials, self.K = particles, log_weights, int(n_trials), int(K)
        self._lse = None

    def __len__(self):
        return self.n_trials

    def lse(self):
        """f32[n_trials][4] = {max, sumexp, lse, lse - log K} per trial (one launch, gjx_trials_lse_pick)"""
        if self._lse is None:
            from .. import kernels
            self._lse, _ = kernels.trials_lse_pick(self.log_weights, self.n_trials, self.K, None, self.particles.prog.rng_mode)
        return self._lse

    def get_log_weights(self):
        return self.log_weights.view(self.n_trials, self.K)

    def moments(self) -> Moments:
        """per-trial posterior means and variances of every choice, each trial normalised on its own: a Moments whose results carry a
        leading ``n_trials`` axis (one gjx_weighted_moments call with n_segments = n_trials, kept)"""
        if getattr(self, "_moments", None) is None:
            self._moments = _moments_of(self.particles, self.log_weights, self.n_trials)
            if self.n_trials == 1:                        # (the kernel wrapper drops a segment axis of 1)
                m = self._moments
                self._moments = Moments(m._trace, m.stats[None], m._mean[None], m._var[None])
        return self._moments

    def quantile(self, addr, q):
        """per-trial weighted quantiles: ``ParticleCollection.quantile`` with a leading ``n_trials`` axis, every trial normalised on
        its own (one gjx_weighted_quantiles call with n_segments = n_trials)"""
        return _quantile_of(self.particles, self.log_weights, addr, q, self.n_trials, 1)

    def probabilities(self, addr):
        """per-trial posterior probabilities of a discrete site: f32[n_trials][2 | ncat] (one call with n_segments = n_trials)"""
        return _probabilities_of(self.particles, self.log_weights, addr, self.n_trials, 1)

    def _pareto(self) -> dict:
        """ONE gjx_pareto_smooth call with n_segments = n_trials for pareto_k() and pareto_smoothed(), kept"""
        if getattr(self, "_psis", None) is None:
            from .. import kernels
            p = kernels.pareto_smooth(self.log_weights, self.n_trials)
            if self.n_trials == 1:                        # (the kernel wrapper drops a segment axis of 1)
                p = dict(p, k=p["k"][None], sigma=p["sigma"][None], cutoff=p["cutoff"][None])
            self._psis = p
        return self._psis

    def pareto_k(self):
        """f32[n_trials]: the Pareto k-hat diagnostic of every trial's weights (``ParticleCollection.pareto_k`` per trial)"""
        return self._pareto()["k"]

    def pareto_smoothed(self) -> "TrialCollections":
        """the same particles under every trial's Pareto-smoothed weights"""
        return TrialCollections(self.particles, self._pareto()["logw"], self.n_trials, self.K)

    def get_log_marginal_likelihood_estimates(self):
        """f32[n_trials]: logsumexp(log_weights of the trial) - log K  (smc.py:96-97 per trial)"""
        return self.lse()[:, 3]

    def trial(self, t: int) -> ParticleCollection:
        """trial t as a ParticleCollection (a copy of its columns)"""
        a, b = t * self.K, (t + 1) * self.K
        tr = self.particles
        sub = Trace(tr.gen_fn, tr.args, tr.prog, tr.choices[:, a:b].contiguous(), tr.score[a:b].contiguous(), tr.shared, True, tr.retval_sym)
        return ParticleCollection(sub, self.log_weights[a:b].contiguous(), True, self.lse()[t], a, self.K)

    def sample_particles(self, key: Key) -> Trace:
        """one particle per trial, drawn 1-of-K over the trial's weights (smc.py:102-109 per trial): a batched Trace of
        n_trials particles"""
        from .. import kernels
        tr = self.particles
        self._lse, pick = kernels.trials_lse_pick(self.log_weights, self.n_trials, self.K, key, tr.prog.rng_mode)
        ch = kernels.gather_rows(tr.choices, pick)
        sc = kernels.gather_rows(tr.score.reshape(1, -1), pick).reshape(-1)
        return Trace(tr.gen_fn, tr.args, tr.prog, ch, sc, tr.shared, True, tr.retval_sym)


class SMCAlgorithm:
    """smc.py:117-225"""

    def get_num_particles(self) -> int:
        raise NotImplementedError

    def get_final_target(self) -> Target:
        raise NotImplementedError

    def run_smc(self, key: Key) -> ParticleCollection:
        raise NotImplementedError

    def run_csmc(self, key: Key, retained: ChoiceMap) -> ParticleCollection:
        raise NotImplementedError

    def log_marginal_likelihood_estimate(self, key: Key, target: Target | None = None):
        algorithm = ChangeTarget(self, target) if target else self
        key, sub_key = split(key)
        return algorithm.run_smc(sub_key).get_log_marginal_likelihood_estimate()

    # GenSP interface
    def random_weighted(self, key: Key, *args: Any):
        target = args[0]
        assert isinstance(target, Target)
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        pc = algorithm.run_smc(key)
        particle = pc.sample_particle(sub_key)
        log_density_estimate = particle.get_score() - pc.get_log_marginal_likelihood_estimate()
        chm = target.filter_to_unconstrained(particle.get_choices())
        return log_density_estimate, chm

    def estimate_logpdf(self, key: Key, v: ChoiceMap, *args: Any):
        target = args[0]
        assert isinstance(target, Target)
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        pc = algorithm.run_csmc(key, v)
        particle = pc.sample_particle(sub_key)
        return particle.get_score() - pc.get_log_marginal_likelihood_estimate()

    def estimate_normalizing_constant(self, key: Key, target: Target):
        algorithm = ChangeTarget(self, target)
        key, sub_key = split(key)
        return algorithm.run_smc(sub_key).get_log_marginal_likelihood_estimate()

    def estimate_reciprocal_normalizing_constant(self, key: Key, target: Target, latent_choices: ChoiceMap, w):
        """smc.py:213-225: ``w`` with ``latent_choices`` is already properly weighted for ``target``, so the retained
        particle skips the reweighting step (ChangeTarget.run_csmc_for_normalizing_constant)."""
        return ChangeTarget(self, target).run_csmc_for_normalizing_constant(key, latent_choices, w)

    def simulate(self, key: Key, args: tuple):
        """Distribution.simulate of an Algorithm (distribution.py:108-115): (score, choices) as a pair."""
        w, chm = self.random_weighted(key, *args)
        return w, chm


def _propose(q, key: Key, target: Target, K: int, offset: int = 0, K_total=None):
    """q.random_weighted vmapped over particles: -> (log_q f32[K], per-particle rows addr -> [dim][K]).
    Properly weighted (log_q = the proposal's full density), unlike the reference's
    Marginal.random_weighted path (sp.py:226-230).  ``offset`` is the global index of this
    rank's first particle: a shard proposes from the same streams the unsharded run would use."""
    gf = q.gen_fn if isinstance(q, Marginal) else q
    tr, out = gf._run(key, K, (target,), ChoiceMap.empty(), True, True, offset=offset, K_total=K_total)
    return out["score"], {a: r for a, r in tr.full_choice_rows().items()}


class ImportanceK(SMCAlgorithm):
    """K-particle importance sampling (smc.py:282-351)."""

    def __init__(self, target: Target, q=None, k_particles: int = 2):
        self.target, self.q, self.k_particles = target, q, int(k_particles)

    def get_num_particles(self):
        return self.k_particles

    def get_final_target(self):
        return self.target

    def run_smc(self, key: Key, offset: int = 0, K_local: int | None = None) -> ParticleCollection:
        """``offset``/``K_local`` select this rank's shard of the K particles (global indices
        [offset, offset + K_local)); the default is the whole collection."""
        K = self.k_particles if K_local is None else int(K_local)
        key, sub_key = split(key)                    # smc.py:299
        # sub_keys = split(sub_key, K) happens on the device: particle i <-> Threefry(sub_key, (0, i))
        if self.q is not None:
            log_q, rows = _propose(self.q, sub_key, self.target, K, offset, self.k_particles)     # smc.py:302-304
            tr, out = self.target.p._run(sub_key, K, self.target.args, self.target.constraint, True, True,
                                         prev_rows=rows, sub=log_q, want_lse=True, offset=offset,
                                         K_total=self.k_particles)
        else:
            # no LSE tail in the producing kernel: its block partials stay in the workspace and are reduced by whoever
            # needs the record first (the resampler's prologue, or one small launch)
            tr, out = self.target.p._run(sub_key, K, self.target.args, self.target.constraint, True, True,
                                         want_lse=False, offset=offset, K_total=self.k_particles)
        return ParticleCollection(tr, out["logw"], True, out["lse"], offset, self.k_particles, partials=out.get("_partials"))

    def run_smc_trials(self, key: Key, n_trials: int) -> TrialCollections:
        """``n_trials`` independent runs of this algorithm in one launch — the device form of the reference idiom
        ``jax.vmap(alg.run_smc)(jax.random.split(key, n_trials))`` (README.md:108-113).  The trials are the consecutive
        K-particle shards of ONE n_trials * K-particle run under ``key`` (counter-based streams: disjoint particle
        indices are independent), each normalised on its own."""
        n, K = int(n_trials), self.k_particles
        key, sub_key = split(key)
        if self.q is not None:
            log_q, rows = _propose(self.q, sub_key, self.target, n * K, 0, n * K)
            tr, out = self.target.p._run(sub_key, n * K, self.target.args, self.target.constraint, True, True,
                                         prev_rows=rows, sub=log_q, want_lse=False, K_total=n * K)
        else:
            tr, out = self.target.p._run(sub_key, n * K, self.target.args, self.target.constraint, True, True,
                                         want_lse=False, K_total=n * K)
        return TrialCollections(tr, out["logw"], n, K)

    def random_weighted_trials(self, key: Key, n_trials: int, *args: Any):
        """``jax.vmap(alg.random_weighted, in_axes=(0, None))(jax.random.split(key, n_trials), target)`` (README.md:110-113)
        in three launches: -> (log-density estimates f32[n_trials], ChoiceMap of the unconstrained choices with a leading
        trial axis)."""
        target = args[0]
        assert isinstance(target, Target)
        key, sub_key = split(key)
        tc = self.run_smc_trials(key, n_trials)
        if not target.same_as(self.target):
            pc = ChangeTarget(self, target)._reweight(key, ParticleCollection(tc.particles, tc.log_weights, True))
            tc = TrialCollections(pc.get_particles(), pc.get_log_weights(), tc.n_trials, tc.K)
        picked = tc.sample_particles(sub_key)
        est = picked.get_score() - tc.get_log_marginal_likelihood_estimates()
        return est, target.filter_to_unconstrained(picked.get_choices())

    def run_csmc(self, key: Key, retained: ChoiceMap) -> ParticleCollection:
        """K-1 fresh particles plus the retained choice map stacked last (smc.py:317-351)."""
        import torch
        K = self.k_particles
        key, sub_key = split(key)
        tgt = self.target
        if self.q is not None:
            log_q, rows = _propose(self.q, sub_key, tgt, K - 1) if K > 1 else (None, {})
            gf = self.q.gen_fn if isinstance(self.q, Marginal) else self.q
            ret_score, _ = gf.assess(retained, (tgt,))
            sl, _ = gf.site_list((tgt,))
            stacked = {}
            for s in sl.sites:
                rv = torch.as_tensor(np.asarray(_host(retained[s.addr]), np.float32).reshape(s.dim, 1), device=ret_score.device)
                stacked[s.addr] = torch.cat([rows[s.addr], rv], dim=1) if K > 1 else rv
            sub = torch.cat([log_q, ret_score.reshape(1)]) if K > 1 else ret_score.reshape(1)
            tr, out = tgt.p._run(key, K, tgt.args, tgt.constraint, True, True, prev_rows=stacked, sub=sub, want_lse=True)
            return ParticleCollection(tr, out["logw"], True, out["lse"])
        # no proposal: K-1 fresh particles from the prior; the retained choices enter as per-particle
        # constraints of a 1-particle run, so both runs share one slot layout and are stacked column-wise
        ret_rows = {}
        sl, _ = tgt.p.site_list(tgt.args)
        for s in sl.sites:
            if s.addr in retained:
                ret_rows[s.addr] = torch.as_tensor(np.asarray(_host(retained[s.addr]), np.float32).reshape(s.dim, 1))
        tr_r, out_r = tgt.p._run(key, 1, tgt.args, tgt.constraint, True, True, prev_rows=ret_rows)
        if K == 1:
            return ParticleCollection(tr_r, out_r["weight"], True)
        tr_f, out_f = tgt.p._run(sub_key, K - 1, tgt.args, tgt.constraint, True, True)
        pf = {a: r for a, r in tr_f.full_choice_rows().items() if tr_r.prog.slot_of[a] >= 0}
        ch = torch.cat([torch.cat([pf[s.addr] for s in sl.sites if tr_r.prog.slot_of[s.addr] >= 0], dim=0), tr_r.choices], dim=1)
        tr = Trace(tgt.p, tgt.args, tr_r.prog, ch.contiguous(), torch.cat([tr_f.score, tr_r.score]), tr_r.shared, True,
                   tr_r.retval_sym)
        return ParticleCollection(tr, torch.cat([out_f["weight"], out_r["weight"]]), True)


class Importance(ImportanceK):
    """1-particle special case (smc.py:233-279)."""

    def __init__(self, target: Target, q=None):
        super().__init__(target, q, 1)


class ChangeTarget(SMCAlgorithm):
    """Reweight an existing collection to a new target (smc.py:359-465)."""

    def __init__(self, prev: SMCAlgorithm, target: Target):
        self.prev, self.target = prev, target

    def get_num_particles(self):
        return self.prev.get_num_particles()

    def get_final_target(self):
        return self.target

    def _reweight(self, key: Key, collection: ParticleCollection) -> ParticleCollection:
        prev_target = self.prev.get_final_target()
        particles = collection.get_particles()
        if self.target.same_as(prev_target):
            # every site would be re-assessed to the same score: this_weight == weight
            return collection
        rows = particles.full_choice_rows()
        latents = {a: r for a, r in rows.items() if a not in prev_target.constraint}   # sp.py:89-91
        K = particles.K
        tr, out = self.target.p._run(key, K, self.target.args, self.target.constraint, True, True, prev_rows=latents,
                                     logw_in=collection.get_log_weights(), sub=particles.score, want_lse=True)
        return ParticleCollection(tr, out["logw"], True, out["lse"])          # smc.py:383: w' - score + w

    def run_smc(self, key: Key) -> ParticleCollection:
        return self._reweight(key, self.prev.run_smc(key))

    def run_csmc(self, key: Key, retained: ChoiceMap) -> ParticleCollection:
        return self._reweight(key, self.prev.run_csmc(key, retained))

    def run_csmc_for_normalizing_constant(self, key: Key, latent_choices: ChoiceMap, w):
        """smc.py:432-465: reciprocal-normalising-constant estimate used by the variational interface — the K-1 fresh
        particles are reweighted to this target, the retained one keeps the caller's weight ``w``."""
        import math
        import torch
        from .. import kernels
        from ..core import split
        key, sub_key = split(key)
        coll = self.prev.run_csmc(sub_key, latent_choices)
        lw = self._reweight(key, coll).get_log_weights().clone()
        retained_score = coll.get_particles().score[-1]
        retained_weight = coll.get_log_weights()[-1]
        lw[-1] = torch.as_tensor(w, dtype=lw.dtype, device=lw.device) - retained_score + retained_weight
        total = kernels.logsumexp(lw.contiguous())[2]
        return retained_score - (total - math.log(self.get_num_particles()))


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else v
