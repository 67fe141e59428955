"""TEST INFRASTRUCTURE ONLY -- the exact per-hand distribution of a rollout whose slots act with
TABLES (nfsp_engine_set_act_table), in float64 numpy over the exported public tree
(``evaluation.GameTree``), for tests/test_act_table.py and tests/test_gpu_act_table.py.  Like
tests/rollout_dist_ref.py it shares nothing with the kernel: no Philox layout, no lookup, no deal.

The walk is rollout_dist_ref's rule 2: per dealer d, ``tree.deal`` at the dealer's root,
``P_PUBLIC`` at chance nodes, the EXECUTED (remapped) table at decisions; ``visit[d][row, rank]``
is the probability that a hand of dealer d reaches the decision of ``row`` with the acting seat
holding ``rank``, and ``reward_mean[d]`` seat 0's expected reward -- ``policy_ref.walk``'s
``value0_dealer{d}`` of the same table at both seats (tests/test_act_table.py asserts that to 1e-12).

``TableModel``: both agents' AR role plays one joint table, sampled (``NFSP_EXT_SAMPLE_AR``), at
eta = 0.  The kernel draws r and takes action 0 if r < y0, 1 if r < y0 + y1 (the sum in float32),
else 2, so the probabilities are (y0, fl(y0 + y1) - y0, 1 - fl(y0 + y1)) of the float32 row.  The
stored action is that draw's one-hot BEFORE the env's raise-to-call remap (rollout_dist_ref's rule
3): ``p_rec[d][row, rank, a] = visit[d][row, rank] x t_raw[row, rank, a]``, while the reach uses
the remapped table.  Every decision leaves exactly one RL record (a one-hot vector is never
all-zero) and, at eta = 0, no SL record.
Not modelled, and why that is safe at 262,144 lanes: the 2^-24 probability of BR mode at eta = 0
(rule 6: 0.03 expected BR-mode seats per rollout) and the 24-bit grid of r (a cell's probability
moves by less than 2^-24: 0.016 counts).  Both move an expectation by less than 0.1 counts.

``eps_greedy_visits``: the least expected number of table-valued records per information set and
lane when both seats play BR tables at eta = 1 with a constant epsilon (test 1's coverage figure).
"""
import numpy as np

from policy_ref import CHANCE, P_PUBLIC, TERMINAL


def sample_probs(rows_f32) -> np.ndarray:
    """P(action) when the kernel samples a float32 row (see the module docstring)."""
    y = np.asarray(rows_f32, np.float32)
    y01 = (y[..., 0] + y[..., 1]).astype(np.float64)
    y0 = y[..., 0].astype(np.float64)
    return np.stack([y0, y01 - y0, 1.0 - y01], axis=-1)


def full_support_table(tree, seed) -> np.ndarray:
    """A seeded float32 table ``[ndec, 3, 3]``: positive rows normalised to 1, the raise column
    positive even where the raise is illegal."""
    rng = np.random.RandomState(seed)
    t = rng.uniform(0.1, 1.0, size=(tree.ndec, 3, 3))
    return (t / t.sum(axis=2, keepdims=True)).astype(np.float32)


def visit_walk(tree, acting):
    """(visit [2, ndec, 3], reward_mean [2], reward_var [2]) under the executed table ``acting``
    (already remapped), per dealer."""
    N = tree.nodes
    seat = tree.seat.astype(int)
    visit = np.zeros((2, tree.ndec, 3))
    m1 = np.zeros(2)
    m2 = np.zeros(2)
    for d in (0, 1):
        reach = np.zeros((tree.nn, 3, 3))                # [node][seat 0's rank][seat 1's rank]
        reach[tree.root[d]] = tree.deal
        for n in range(tree.nn):                         # depth order: parents first
            par = int(N["parent"][n])
            if par >= 0:
                via = int(N["via"][n])
                if N["kind"][par] == CHANCE:
                    reach[n] = reach[par] * P_PUBLIC[via]
                else:
                    col = acting[int(N["row"][par])][:, via]
                    reach[n] = reach[par] * (col[:, None] if N["p"][par] == 0 else col[None, :])
            if N["kind"][n] == TERMINAL:
                pay = tree.pay[int(N["row"][n]), 0].astype(np.float64)
                m1[d] += float((reach[n] * pay).sum())
                m2[d] += float((reach[n] * pay * pay).sum())
        at = reach[tree.node_of_row]                     # [ndec, 3, 3]
        visit[d] = np.where((seat == 0)[:, None], at.sum(axis=2), at.sum(axis=1))
    return visit, m1, m2 - m1 * m1


class TableModel:
    """The model of the module docstring for the float32 joint table ``rows``; duck-typed to
    what ``rollout_dist_ref._cells`` and ``check_counts`` read of a ``Model``'s RL side."""

    def __init__(self, tree, rows):
        self.tree = tree
        self.seat = tree.seat.astype(int)
        self.dealer_of_row = np.array([tree.path(r)[0] for r in range(tree.ndec)])
        self.t_raw = sample_probs(np.asarray(rows, np.float32).reshape(tree.ndec, 3, 3))
        self.acting = tree.remap(self.t_raw)
        self.visit, self.reward_mean, self.reward_var = visit_walk(tree, self.acting)
        self.p_rec = self.visit[:, :, :, None] * self.t_raw[None]


def eps_greedy_visits(tree, rows, eps) -> np.ndarray:
    """[ndec, 3]: per lane, the expected number of decisions at each information set that act with
    the table's row (the epsilon draw does not fire), when both seats play ``rows`` greedily in BR
    mode with a constant ``eps`` -- the acting table is (1 - eps) x one-hot(first maximum) + eps x
    uniform over three actions, remapped; dealers 0 and 1 are equally likely."""
    y = np.asarray(rows, np.float64).reshape(tree.ndec, 3, 3)
    mixed = (1.0 - eps) * np.eye(3)[np.argmax(y, axis=2)] + eps / 3.0
    visit, _, _ = visit_walk(tree, tree.remap(mixed))
    return 0.5 * (visit[0] + visit[1]) * (1.0 - eps)


def lookup_table(tree, seed) -> np.ndarray:
    """Test 1's rows: v[a] = 2 + (9 row + 3 rank + a) / 4096, the three values of every (row, rank)
    permuted by a seeded choice so that the argmax varies.  All >= 2, unique, exact in float32."""
    rng = np.random.RandomState(seed)
    v = 2.0 + np.arange(tree.ndec * 9, dtype=np.float64).reshape(tree.ndec, 3, 3) / 4096.0
    out = np.empty_like(v)
    for d in range(tree.ndec):
        for r in range(3):
            out[d, r] = v[d, r][rng.permutation(3)]
    t = out.astype(np.float32)
    assert np.array_equal(t.astype(np.float64), out) and len(np.unique(t)) == t.size and t.min() >= 2.0
    return t
