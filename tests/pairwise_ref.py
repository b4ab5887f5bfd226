"""float64 NumPy restatement of gjx_pairwise_gauss_lse (the direct |q - k|^2 form, not the kernel's expansion), of the FFBSm recursion
on it, and the bound the GPU tests hold the kernel to.  Per output r (u = 2^-24, tildes: minus the call's centre, maximum over LIVE keys):
    C u (d + C0) p (|q~_r|^2 + max_c |k~_c|^2)  +  C1 u (1 + log n_k)
First term: the kernel adds -1/2 p |q~|^2, bias - 1/2 p |k~|^2 and p q~ . k~ in float32, each a d-term sum of magnitude at most
p (|q~|^2 + |k~|^2) / 2 with d + a few roundings; C0 = 4: the scalings by p and log2 e and the additions that join the three.  Second
term: a score s is a float32 number with error u |s|, and the bias enters as it is; biases are log-weights (normalised: log n_k and a
few), the log-sum-exp adds log n_k of its own: C1 = 8 covers |bias| <= 8 (1 + log n_k), where the tests stay, and the 1-ulp hardware
exp and log.  C is the one measured constant; the tests use 4 x the measurement, as affine_sites_ref.py does with C_ELEM."""
import numpy as np

U = 2.0 ** -24
C0, C1 = 4.0, 8.0
C_MEASURED = 0.125            # worst error / bound(C = 1) on an MI355X: 0.120 (d = 1, n_q = 17, n_k = 194, no bias), rounded up
C = 4.0 * C_MEASURED


def _live(bias, n_k):
    b = np.zeros(n_k) if bias is None else np.asarray(bias, np.float64)
    return b, b > -np.inf                                   # (False for -inf and for NaN)


def pairwise_lse(q, k, bias, p):
    """q f64[d][n_q], k f64[d][n_k], bias [n_k] or None -> f64[n_q]; dead keys are left out whatever they hold"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    b, live = _live(bias, k.shape[1])
    out = np.full(q.shape[1], -np.inf)
    if live.any():
        s = b[live][None, :] - 0.5 * p * ((q[:, :, None] - k[:, None, live]) ** 2).sum(0)
        m = s.max(1)
        out = m + np.log(np.exp(s - m[:, None]).sum(1))
    return np.where(np.isfinite(q).all(0), out, np.nan)


def bound(q, k, bias, p, centre=None, c=C):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    cen = np.zeros((q.shape[0], 1)) if centre is None else np.asarray(centre, np.float64).reshape(-1, 1)
    _, live = _live(bias, k.shape[1])
    k2 = ((k[:, live] - cen) ** 2).sum(0).max() if live.any() else 0.0
    return c * U * (q.shape[0] + C0) * p * (((q - cen) ** 2).sum(0) + k2) + C1 * U * (1.0 + np.log(k.shape[1]))


def ffbs_log_weights(states, logw, means, p):
    """the FFBSm recursion in float64 -> log w_{t|T}, f64[T][K], every row normalised"""
    norm = lambda lw: lw - np.logaddexp.reduce(lw)
    T = len(states)
    out = [None] * T
    out[T - 1] = norm(np.asarray(logw[T - 1], np.float64))
    for t in range(T - 2, -1, -1):
        lw = norm(np.asarray(logw[t], np.float64))
        D = pairwise_lse(states[t + 1], means[t], lw, p)
        out[t] = norm(lw + pairwise_lse(means[t], states[t + 1], out[t + 1] - D, p))
    return np.stack(out)
