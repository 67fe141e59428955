"""TEST INFRASTRUCTURE ONLY -- the numpy restatement of regret nets on the MCCFR handle
(csrc/mccfr.hip k_mccfr_net_apply), wrapped around mccfr_x_ref.XRef of the three sampling kinds
without touching them.  The rule (include/nfsp.h, "regret nets on the same handle"):

A run has two packed 30-64-3 nets w[seat] with linear heads and their momentum states v[seat]
(0 at the start).  Steps 1 to 3 are XRef's, with one change: the sigma a half-iteration reads is
the nets'.  After the tables of a half-iteration of seat i are applied, for seat i, with
tw = (double)(t + 1):

  targets  AVG     y_a = (double)R_a / (((double)W * Q) * tw)
           ROWMAX  m = max |R_b| over the legal b (int64); y_a = (double)R_a / (double)m, 0 where m = 0
           an illegal raise has y = 0 (and the fit's default mask removes it)
  fit      K steps of fitnet_ref.fit (nfsp_fit_tables' step), uniform weights, the linear head,
           from (w[i], v[i]), which carry over
  head     z[d][r][.] = the net's head sums at the seat's rows, f32
  sigma    rp_a = max((double)z_a, 0), 0 at an illegal raise; sigma = the row normalisation of
           regret matching (uniform over the legal actions where the sum is 0)

At the start both seats take the step once with R = 0 and tw = 1.  The regret-matching table on R
is kept beside (``sigma_tab``).

Two hooks.  ``sigma_hook(i)``, when set, supplies the [ndec, 3, 3] sigma that half-iteration i
reads: an f32 difference of 1e-7 between two nets can flip a sampled choice, so a comparison with
the device is teacher-forced.  ``head_hook(i, y)``, when set, replaces fit and head: it returns
the seat's z [N, 3] from the targets y [ndec, 3, 3] (f64), in any dtype.
"""
import numpy as np

import fitnet_ref as fr
import mccfr_ref as mr
import mccfr_x_ref as xr
import policy_ref as pr

AVG, ROWMAX = 0, 1
_CLASSES = {}


def targets(tree, R, walkers, tw, kind):
    """y [ndec, 3, 3] in f64 from the int64 regrets."""
    R = np.asarray(R, np.int64)
    legal = np.ones(R.shape, bool)
    legal[~tree.legal, :, 2] = False
    Rl = np.where(legal, R, 0)
    if kind == AVG:
        den = (np.float64(walkers) * mr.Q) * np.float64(tw)
        y = Rl.astype(np.float64) / den
    else:
        m = np.abs(Rl).max(axis=2, keepdims=True)
        y = np.where(m > 0, Rl.astype(np.float64) / np.where(m > 0, m, 1).astype(np.float64), 0.0)
    return np.where(legal, y, 0.0)


def sigma_of(tree, z):
    """sigma [ndec, 3, 3] from heads z (any float dtype): regret matching in f64."""
    rp = np.maximum(np.asarray(z).astype(np.float64), 0.0)
    rp[~tree.legal, :, 2] = 0.0
    return pr.average_rows(tree, rp)


def NetRef(base):
    """The class of runs of sampling kind ``base`` with regret nets: ``NetRef(OsRef)(tree, seed, W, eps,
    nets=(w0, w1), target=AVG, fit_steps=K, loss=fr.MSE, lr=0.5, momentum=0.9)``."""
    if base in _CLASSES:
        return _CLASSES[base]

    class N(xr.XRef(base)):
        def __init__(self, *args, nets, target=AVG, fit_steps=0, loss=fr.MSE, lr=0.5, momentum=0.9,
                     head_hook=None, **kw):
            super().__init__(*args, **kw)
            assert target in (AVG, ROWMAX) and loss in (fr.MSE, fr.HUBER) and fit_steps >= 0
            self.target, self.K, self.loss, self.lr, self.mu = target, int(fit_steps), loss, lr, momentum
            self.w = [np.array(nets[0], np.float32), np.array(nets[1], np.float32)]
            self.v = [np.zeros(fr.NP, np.float32), np.zeros(fr.NP, np.float32)]
            self.z = np.zeros(self.R.shape, np.float32)
            self.sg = np.zeros(self.R.shape, np.float64)
            self.fit_loss = np.zeros((2, 2))
            self.sigma_hook, self.head_hook = None, head_hook
            self._reading = None
            for i in (0, 1):
                self.net_step(i, 1.0)

        def sigma(self):
            if self.sigma_hook is not None and self._reading is not None:
                return np.asarray(self.sigma_hook(self._reading), np.float64)
            return self.sg

        def sigma_tab(self):
            return mr.match(self.tree, self.R)

        def net_step(self, i, tw):
            y = targets(self.tree, self.R, self.W, tw, self.target)
            d, r = fr.seat_sets(self.tree, i)
            if self.head_hook is not None:
                z = np.asarray(self.head_hook(i, y))
                self.z = self.z.astype(np.result_type(self.z.dtype, z.dtype))
            else:
                prob = fr.problem(self.tree, i, y)
                self.w[i], self.v[i], self.fit_loss[i] = fr.fit(self.w[i], prob, fr.ACT_LINEAR, self.loss, self.lr,
                                                               self.mu, self.K, v0=self.v[i])
                z = fr.forward(self.w[i], prob[0])[2]
            self.z[d, r] = z
            self.sg[d, r] = sigma_of(self.tree, self.z)[d, r]

        def half(self, i):
            self._reading = i
            super().half(i)                                  # the walk with self.sigma(), then XRef's step 3
            self._reading = None
            self.net_step(i, float(self.t + 1))

    N.__name__ = "Net" + base.__name__
    _CLASSES[base] = N
    return N
