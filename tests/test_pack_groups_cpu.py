"""Host logic of `apply_batch(pack=...)`: which files share a launch group (pipelining.PackGrouper / pack_groups).

Files are joined greedily, in input order, while the group's total chunk count stays within the budget; a file that
alone exceeds the budget is a group of its own; the incremental form (a file's chunk count is known only once the file
is loaded) forms the groups the all-at-once form does.  No torch, no GPU."""
import random

import pytest

from pyannote_audio_amd.pipelining import PackGrouper, pack_groups


def _check(sizes, budget, groups):
    assert [i for g in groups for i in g] == list(range(len(sizes)))          # every file once, order kept
    assert all(g for g in groups)
    for g in groups:
        total = sum(sizes[i] for i in g)
        assert total <= budget or len(g) == 1                                 # only a single file may exceed it
    for g, h in zip(groups[:-1], groups[1:]):                                 # greedy: the next file did not fit
        assert sum(sizes[i] for i in g) + sizes[h[0]] > budget


def test_order_and_budget():
    sizes = [24, 3, 18, 1, 6, 1, 40, 40, 2]
    groups = pack_groups(sizes, 48)
    assert groups == [[0, 1, 2, 3], [4, 5, 6], [7, 8]]
    _check(sizes, 48, groups)
    assert pack_groups([10, 10, 10], 30) == [[0, 1, 2]]                       # exactly the budget still fits
    assert pack_groups([10, 10, 11], 30) == [[0, 1], [2]]


def test_an_oversize_file_is_a_group_of_its_own():
    assert pack_groups([100], 16) == [[0]]
    assert pack_groups([3, 100, 4], 16) == [[0], [1], [2]]                    # between small ones: nothing joins it
    assert pack_groups([3, 4, 100, 100, 5, 6], 16) == [[0, 1], [2], [3], [4, 5]]
    assert pack_groups([100, 1], 16) == [[0], [1]]
    _check([3, 4, 100, 100, 5, 6], 16, pack_groups([3, 4, 100, 100, 5, 6], 16))


def test_budget_one_and_empty_input():
    assert pack_groups([1, 1, 1], 1) == [[0], [1], [2]]
    assert pack_groups([2, 1, 3], 1) == [[0], [1], [2]]
    assert pack_groups([], 8) == []
    assert pack_groups(iter([]), 1) == []
    grouper = PackGrouper(8)
    assert grouper.flush() == []
    with pytest.raises(ValueError):
        PackGrouper(0)
    with pytest.raises(ValueError):
        PackGrouper(4).add(-1)


def test_files_without_chunks_join_their_neighbours():
    assert pack_groups([0, 4, 0, 4, 0], 8) == [[0, 1, 2, 3, 4]]
    assert pack_groups([0, 0], 1) == [[0, 1]]


def test_incremental_form_agrees_with_the_all_at_once_form():
    rng = random.Random(7)
    for _ in range(300):
        n = rng.randrange(0, 40)
        budget = rng.choice([1, 2, 5, 16, 64, 4096])
        sizes = [rng.choice([0, 1, 1, 2, 3, 21, 30, 70, 5000]) for _ in range(n)]
        want = pack_groups(sizes, budget)
        _check(sizes, budget, want)
        grouper, got, seen = PackGrouper(budget), [], 0
        for size in sizes:
            closed = grouper.add(size)
            if closed is not None:
                # a group is handed out as soon as the first file that does not fit arrives -- and not before
                assert closed == list(range(seen, seen + len(closed)))
                seen += len(closed)
                got.append(closed)
        last = grouper.flush()
        if last:
            got.append(last)
        assert got == want
        assert grouper.flush() == []                                          # nothing is handed out twice
