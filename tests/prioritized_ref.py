"""NumPy float64 restatement of the priority tree (tonic_amd/csrc/priority.hip, include/tonic_hip.h): the same levels
with explicit ascending sums, the same descent rule, the importance weights and the update with the highest batch
position winning a repeated index.  Shared by the prioritized-replay tests; nothing here touches a GPU."""
import numpy as np


def pad64(n):
    return (n + 63) // 64 * 64


def level_sizes(capacity):
    """Nodes per level, leaves first; the levels stop at the first one with <= 64 nodes."""
    sizes = [capacity]
    while sizes[-1] > 64:
        sizes.append((sizes[-1] + 63) // 64)
    return sizes


def tree_bytes(capacity):
    sizes = level_sizes(capacity)
    return 64 + 4 * pad64(sizes[0]) + sum(8 * pad64(n) for n in sizes[1:])


def level_offsets(capacity):
    """Byte offset of every level in the device block (the float32 max_leaf sits at byte 0)."""
    sizes, offsets, end = level_sizes(capacity), [], 64
    for level, n in enumerate(sizes):
        offsets.append(end)
        end += (4 if level == 0 else 8) * pad64(n)
    return offsets


def ascending_sums(children):
    """[nodes, 64] -> [nodes]: each row summed in ascending order (np.sum would add pairwise)."""
    return np.cumsum(children, axis=-1)[..., -1]


class Tree:
    """levels[0]: the leaves as float64 [pad64(capacity)]; levels[l]: float64 [pad64(n_l)], zero behind n_l."""

    def __init__(self, capacity, leaves=None, max_leaf=1.0):
        self.capacity, self.sizes = capacity, level_sizes(capacity)
        self.levels = [np.zeros(pad64(n), np.float64) for n in self.sizes]
        self.max_leaf = np.float32(max_leaf)
        if leaves is not None:
            self.levels[0][:capacity] = np.asarray(leaves, np.float64)
            self.rebuild()

    def rebuild(self):
        for level in range(1, len(self.levels)):
            sums = ascending_sums(self.levels[level - 1].reshape(-1, 64))
            self.levels[level][:len(sums)] = sums

    @property
    def leaves(self):
        return self.levels[0][:self.capacity]

    @property
    def total(self):
        return np.cumsum(self.levels[-1][:64])[-1]

    def descend(self, u):
        """(index, margin): the drawn leaf, and the smallest distance of the running target from a prefix boundary
        of a scanned node, as a fraction of the total (how far rounding is from changing the outcome)."""
        target, node, margin = u * self.total, 0, np.inf
        for level in range(len(self.levels) - 1, -1, -1):
            children = self.levels[level][node * 64:node * 64 + 64]
            inclusive = np.cumsum(children)
            margin = min(margin, np.abs(inclusive - target).min() / self.total)
            above = np.flatnonzero(inclusive > target)
            if len(above):
                child = int(above[0])
            else:
                live = np.flatnonzero(children > 0)
                child = int(live[-1]) if len(live) else 0
            if child > 0:
                target = target - inclusive[child - 1]
            node = node * 64 + child
        return node, margin

    def sample(self, uniforms):
        return np.array([self.descend(u)[0] for u in uniforms], np.int64)

    def weights(self, indices, beta):
        drawn = self.leaves[indices]
        return (drawn.min() / drawn) ** beta

    def store(self, first, count):
        self.levels[0][first:first + count] = np.float64(self.max_leaf)
        self.rebuild()

    def update(self, indices, losses, alpha, epsilon):
        """float32 inputs; the leaf is what float32 holds of (loss + epsilon)^alpha computed in float64 from the
        float32 sum.  A later batch position overwrites an earlier one."""
        base = np.maximum(np.asarray(losses, np.float32) + np.float32(epsilon), np.float32(0))
        new = (base.astype(np.float64) ** np.float64(np.float32(alpha))).astype(np.float32)
        written = {}
        for index, leaf in zip(indices, new):
            if 0 <= index < self.capacity:
                written[int(index)] = leaf
        for index, leaf in written.items():
            self.levels[0][index] = np.float64(leaf)
        if written:
            self.max_leaf = max(self.max_leaf, np.float32(max(written.values())))
        self.rebuild()
        return written


def safe_uniforms(tree, count, rng, keep=(), margin=1e-9):
    """`count` uniforms chosen from this float64 reference alone: every draw's target lies at least `margin` * total
    from every prefix boundary on its path — the float64 association-order error of the device's sums is below
    levels * 64 * 2^-53 * total (about 3e-14), so the margin is 10^4 times that bound.  A draw closer than that is
    REPLACED by a fresh one, never skipped; `keep` (u = 0, u = 1 - 2^-53) go first and stay whatever their margin:
    their outcomes, the first and the last non-zero leaf, must hold regardless."""
    out = list(keep)[:count]
    while len(out) < count:
        u = rng.random_sample()
        if tree.descend(u)[1] >= margin:
            out.append(u)
    return np.array(out, np.float64)
