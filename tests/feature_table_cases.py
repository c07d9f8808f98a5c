"""The occurrence patterns that test_feature_table_cpu.py and test_gpu_feature_table.py share: a table of 37 rows, two sides of occurrence
ids with their gradient rows, drawn from fixed seeds."""
import numpy as np

N_ROWS = 37
D_VALUES = (1, 7, 250, 513)
SPLIT = 64                  # feature_table.SPLIT: the longest segment one wave sums alone


def _ids(case, rng):
    """(ids_a, ids_b) as int64 arrays"""
    r = lambda n: rng.randint(0, N_ROWS, n)
    if case == "all_distinct":
        p = rng.permutation(N_ROWS)
        return p[:25], p[25:]
    if case == "duplicates":
        return r(300), r(41)
    if case == "one_id_2100":                   # one long segment, far over the split threshold
        return np.full(2000, 11), np.full(100, 11)
    if case == "just_under_split":              # 64 occurrences of row 5: the longest segment a single wave sums
        return np.concatenate([np.full(SPLIT - 4, 5), r(30) % 5]), np.full(4, 5)
    if case == "just_over_split":               # 65: the shortest split segment (13 slices of 5)
        return np.concatenate([np.full(SPLIT - 3, 5), r(30) % 5]), np.full(4, 5)
    if case == "mixed_lengths":                 # long and short segments in one tile, and more than one tile of segments
        return np.concatenate([np.full(200, 3), np.full(70, 20), r(150), np.full(129, 36)]), np.concatenate([r(60), np.full(90, 0)])
    if case == "first_and_last_row":
        return np.array([0, 36, 36, 0, 0]), np.array([36, 0])
    if case == "same_id_both_sides":            # a's occurrences come before b's
        return np.array([9, 9, 4, 9]), np.array([9, 4, 9])
    if case == "a_empty":
        return np.zeros(0, np.int64), r(50)
    if case == "b_empty":
        return r(50), np.zeros(0, np.int64)
    if case == "both_empty":
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if case == "out_of_range":                  # about 10 % of the ids outside [0, 37): negative, just past the end, far past it
        a, b = r(400), r(60)
        bad = np.array([-1, -7, N_ROWS, N_ROWS + 1, 1000, 2 ** 31 - 1, -2 ** 31])
        for ids in (a, b):
            hit = rng.rand(len(ids)) < 0.1
            ids[hit] = bad[rng.randint(0, len(bad), int(hit.sum()))]
        return a, b
    if case == "trainable_mask":
        return r(300), r(41)
    raise KeyError(case)


CASES = ("all_distinct", "duplicates", "one_id_2100", "just_under_split", "just_over_split", "mixed_lengths", "first_and_last_row",
         "same_id_both_sides", "a_empty", "b_empty", "both_empty", "out_of_range", "trainable_mask")


def draw_case(case, d, seed=0):
    """dict(ids_a, ids_b int64; d_a [n_a, d], d_b [n_b, d] float32 with magnitudes spread over six decades; trainable uint8 [37] or
    absent)"""
    rng = np.random.RandomState(1000 * seed + CASES.index(case))
    ids_a, ids_b = (np.asarray(i, dtype=np.int64) for i in _ids(case, rng))
    grad = lambda n: (rng.randn(n, d) * 10.0 ** rng.randint(-3, 3, (n, 1))).astype(np.float32)
    out = dict(ids_a=ids_a, ids_b=ids_b, d_a=grad(len(ids_a)), d_b=grad(len(ids_b)))
    if case == "trainable_mask":
        out["trainable"] = (rng.rand(N_ROWS) < 0.6).astype(np.uint8)
    return out


def draw_state(d, amsgrad, seed=0):
    """(weight, exp_avg, exp_avg_sq, max_exp_avg_sq or None) [37, d] float32: the state after some earlier steps (vmax >= v)"""
    rng = np.random.RandomState(77 + seed)
    w = rng.randn(N_ROWS, d).astype(np.float32)
    m, v = (0.1 * rng.randn(N_ROWS, d)).astype(np.float32), (rng.rand(N_ROWS, d) ** 2).astype(np.float32)
    x = np.maximum(v, rng.rand(N_ROWS, d).astype(np.float32)) if amsgrad else None
    return w, m, v, x
