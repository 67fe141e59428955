"""TEST INFRASTRUCTURE ONLY -- the numpy restatement of regret matching+ and linear averaging on
the MCCFR handle (csrc/mccfr.hip k_mccfr_x_apply), wrapped around the restatements of the three
sampling kinds (mccfr_ref.MccfrRef, mccfr_os_ref.OsRef, mccfr_vr_ref.VrRef) without touching them.
The rule (include/nfsp.h, "regret matching+ and linear averaging"):

Steps 1 and 2 of a half-iteration are the sampling kind's own -- so dR and dS are taken here as
what the base restatement's half-iteration added to R and S.  Step 3, t the iterations completed
before the one in progress (the same for both of its half-iterations), per entry and in this order:

  R = R + dR, and under REGRET_PLUS then R = max(R, 0)          int64
  S = S + dS                                                   int64
  Sw = Sw + (double)(t + 1) * (double)dS                       f64: one product, one sum

The next sigma comes from the new R by the unchanged regret matching.  The uniform average is the
base's, from (double)S; the linear one is the same normalisation of Sw.
"""
import numpy as np

import policy_ref as pr

PLAIN, PLUS = 0, 1
UNIFORM, LINEAR = 0, 1
_CLASSES = {}


def XRef(base):
    """The class of runs of sampling kind ``base`` under the rule: ``XRef(VrRef)(tree, seed, W, eps,
    regret=PLUS, average=LINEAR)``.  The base's arguments come first, as the base takes them."""
    if base in _CLASSES:
        return _CLASSES[base]

    class X(base):
        def __init__(self, *args, regret=PLAIN, average=UNIFORM, **kw):
            super().__init__(*args, **kw)
            assert regret in (PLAIN, PLUS) and average in (UNIFORM, LINEAR)
            self.regret, self.avg = regret, average
            self.Sw = np.zeros(self.S.shape, np.float64)

        def half(self, i):
            R0, S0 = self.R.copy(), self.S.copy()
            super().half(i)                                  # R += dR, S += dS (and the baseline's sums)
            dS = self.S - S0
            assert np.array_equal(self.R - R0 + R0, self.R)  # dR = R - R0 did not wrap
            if self.regret == PLUS:
                self.R = np.maximum(self.R, 0)
            self.Sw = self.Sw + np.float64(self.t + 1) * dS.astype(np.float64)

        def average(self, which=None):
            which = self.avg if which is None else which
            return pr.average_rows(self.tree, self.Sw if which == LINEAR else self.S.astype(np.float64))

    X.__name__ = "X" + base.__name__
    _CLASSES[base] = X
    return X
