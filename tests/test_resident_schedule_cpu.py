"""The arithmetic of Estimator.train_resident as pure functions (no device): which graphs a call replays
(estimator.resident_schedule) and how a graph's steps are cut into optimizer windows (estimator.window_lengths)."""
import pytest

from recsys_amd.estimator import resident_schedule, window_lengths


@pytest.mark.parametrize("n,spg,start,steps,expected", [
    (16, 16, 2, 18, [(2, 14, "head"), (0, 4, "tail")]),      # the first call: two eager warm-up steps leave the stream at batch 2
    (16, 16, 0, 20, [(0, 16, "group"), (0, 4, "tail")]),     # the tail would wrap: a graph of its own
    (32, 16, 0, 20, [(0, 20, "tail")]),                      # a full group + a tail shorter than half a group: ONE graph
    (8, 4, 0, 5, [(0, 5, "tail")]),
])
def test_schedule_worked_cases(n, spg, start, steps, expected):
    assert resident_schedule(start, steps, n, spg) == expected


@pytest.mark.parametrize("count,K,expected", [(20, 8, [7, 7, 6]), (16, 8, [8, 8]), (5, 8, [5])])
def test_window_lengths_worked_cases(count, K, expected):
    assert window_lengths(count, K) == expected


@pytest.mark.parametrize("n", [8, 16, 32])
@pytest.mark.parametrize("spg", [4, 8, 16])
@pytest.mark.parametrize("start", [0, 2])
def test_schedule_covers_the_steps_in_order(n, spg, start):
    for steps in range(1, 41):
        sched = resident_schedule(start, steps, n, spg)
        where = (n, spg, start, steps, sched)
        assert sum(c for _, c, _ in sched) == steps, where
        pos = start % n
        for first, count, kind in sched:
            assert first == pos and count > 0 and kind in ("head", "group", "tail"), where
            pos = (pos + count) % n
        kinds = [k for _, _, k in sched]
        assert kinds.count("head") <= 1 and kinds.count("tail") <= 1, where
        assert kinds == sorted(kinds, key=("head", "group", "tail").index), where        # head, groups, tail: in this order
        for first, count, kind in sched:
            if kind == "group":
                assert count == spg and first % spg == 0, where
            elif kind == "head":       # up to the next group boundary, unless the steps run out before it
                assert first % spg and count < spg and ((first + count) % spg == 0 or len(sched) == 1), where
            elif count > spg:          # the merged tail: one full group + less than half a group, which does not wrap
                assert first % spg == 0 and count < spg + spg // 2 and first + count <= n, where
            assert kind == "tail" or count <= spg, where


def test_window_lengths_are_even_and_bounded():
    for K in range(1, 9):
        for count in range(1, 41):
            w = window_lengths(count, K)
            assert sum(w) == count and max(w) <= K and max(w) - min(w) <= 1, (count, K, w)
            assert len(w) == -(-count // K) and w == sorted(w, reverse=True), (count, K, w)
