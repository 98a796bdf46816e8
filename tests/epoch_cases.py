"""Inputs and the brute-force reference shared by tests/test_epoch_host.py and tests/test_gpu_epoch.py."""
import numpy as np
import torch

# n = 12, E = 30: every kind of row the reference's rule distinguishes
HAND_N = 12
HAND_ROWS = [
    (0, 1), (0, 1),                      # 0, 1     a pair repeated in the same direction
    (2, 3), (3, 2),                      # 2, 3     a pair present as (u, v) and (v, u)
    (4, 5), (5, 4), (4, 5),              # 4, 5, 6  a triple -- the mixed batch holds two of its rows
    (6, 7), (6, 7), (7, 6),              # 7, 8, 9  a triple -- the mixed batch holds all three
    (8, 8),                              # 10       a self-loop row
    (0, 2), (0, 3), (1, 2), (1, 3), (2, 4), (2, 5), (3, 6), (3, 7), (4, 8), (5, 9), (6, 10), (7, 11), (8, 9), (9, 10),
    (10, 11), (11, 0), (10, 1), (9, 11), (5, 8),      # 11 .. 29  ordinary unique rows, two of them with u > v
]
HAND_MIXED = [20, 9, 0, 3, 4, 15, 7, 10, 2, 5, 26, 8, 11]
HAND_BATCHES = {"empty": [], "one_row": [12], "one_of_two": [1], "all_rows": list(range(len(HAND_ROWS))),
                "mixed": HAND_MIXED}


def hand_train_pos() -> torch.Tensor:
    return torch.tensor(HAND_ROWS, dtype=torch.int64)


def brute_force_removed(train_pos, perm) -> set:
    """The reference's rule, literally: the rows NOT in the batch -> their set of undirected pairs; what the batch
    removes is the complement within the pairs of all rows."""
    rows = [tuple(sorted(r)) for r in np.asarray(train_pos).tolist()]
    batch = set(int(i) for i in np.asarray(perm).reshape(-1).tolist())
    kept = {p for i, p in enumerate(rows) if i not in batch}
    return set(rows) - kept


def brute_force_covered(train_pos, perm) -> np.ndarray:
    """[2, B]: (min, max) of row perm[i] where its pair is removed, else (-1, -1); ids outside [0, E): (-1, -1)."""
    tp = np.asarray(train_pos)
    perm = np.asarray(perm).reshape(-1)
    inside = [int(i) for i in perm.tolist() if 0 <= i < tp.shape[0]]
    removed = brute_force_removed(tp, inside)
    out = np.full((2, perm.size), -1, np.int64)
    for i, r in enumerate(perm.tolist()):
        if 0 <= r < tp.shape[0]:
            p = tuple(sorted(tp[r].tolist()))
            if p in removed:
                out[:, i] = p
    return out


def symmetric_keys(train_pos, n: int) -> torch.Tensor:
    """Sorted distinct directed keys row * n + col of the symmetrised rows (numpy, independent of TrainEdges)."""
    tp = np.asarray(train_pos).astype(np.int64)
    return torch.from_numpy(np.unique(np.concatenate([tp[:, 0] * n + tp[:, 1], tp[:, 1] * n + tp[:, 0]])))


class AdjacencyStandIn:
    """What ``TrainEdges.check_against`` reads of a model."""

    def __init__(self, keys: torch.Tensor, n: int):
        self.keys, self.num_nodes = keys, n

    def _own_mask_keys(self, test_set):
        return self.keys


def random_rows_with_duplicates(E: int, n: int, seed: int) -> torch.Tensor:
    """E rows over n nodes: a quarter of them copies of other rows, half of those reversed; shuffled."""
    rng = np.random.default_rng(seed)
    n_dup = E // 4
    base = rng.integers(0, n, (E - n_dup, 2))
    dup = base[rng.choice(E - n_dup, n_dup, replace=False)].copy()
    dup[: n_dup // 2] = dup[: n_dup // 2, ::-1]
    rows = np.concatenate([base, dup])
    return torch.from_numpy(rows[rng.permutation(E)].astype(np.int64))
