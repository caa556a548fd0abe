"""ada_mvs_amd/cloud_lattice.py without a device: the cut of sorted query keys into work items against a plain loop, and the keyed,
sorted cloud.  Both are plain torch, so CPU tensors stand for the device's here; cloud_filter.Search and accuracy.nearest run the
same functions on the device's keys."""
import numpy as np
import torch

import ada_mvs_amd  # noqa: F401
from ada_mvs_amd import _lib, cloud_lattice

TOP = (1 << 63) - 1
RUNS = (1, 255, 256, 257, 513)


def loop_items(sorted_keys):
    """The work items by the rule in words: the keys of -1 first and set aside; every run of equal keys cut front to back into
    pieces of CLOUD_TILE, the last piece what is left; first counts from the first key >= 0."""
    keys = [int(k) for k in sorted_keys]
    outside = sum(1 for k in keys if k < 0)
    items, at = [], outside
    while at < len(keys):
        end = at
        while end < len(keys) and keys[end] == keys[at]:
            end += 1
        for first in range(at, end, _lib.CLOUD_TILE):
            items.append((keys[at], first - outside, min(_lib.CLOUD_TILE, end - first)))
        at = end
    return outside, items


def runs_of(keys):
    return torch.tensor([k for k, n in zip(keys, RUNS) for _ in range(n)], dtype=torch.int64)


def as_list(items):
    return list(zip(*(t.tolist() for t in items)))


def check(sorted_keys):
    order = torch.randperm(sorted_keys.numel(), generator=torch.Generator().manual_seed(3))
    outside, qorder, items = cloud_lattice.work_items(sorted_keys, order)
    want_outside, want = loop_items(sorted_keys)
    assert outside == want_outside and torch.equal(qorder, order[want_outside:])
    if not want:
        assert items is None
        return outside, []
    assert items[0].dtype == items[1].dtype == torch.int64 and items[2].dtype == torch.int32
    assert as_list(items) == want
    return outside, want


def test_runs_around_the_tile_are_cut_as_the_plain_loop_cuts_them():
    outside, items = check(runs_of((3, 7, 8, 1 << 21, 1 << 42)))
    assert outside == 0
    per_key = {k: [c for key, _, c in items if key == k] for k in (3, 7, 8, 1 << 21, 1 << 42)}
    assert [len(v) for v in per_key.values()] == [1, 1, 1, 2, 3]
    assert per_key[1 << 21] == [256, 1] and per_key[1 << 42] == [256, 256, 1]


def test_keys_outside_the_lattice_come_first_and_are_skipped():
    outside, items = check(torch.cat([torch.full((3,), -1, dtype=torch.int64), runs_of((3, 7, 8, 1 << 21, 1 << 42))]))
    assert outside == 3 and items[0] == (3, 0, 1)


def test_the_largest_key_is_a_run_like_any_other():
    outside, items = check(runs_of((0, 5, 6, TOP - 1, TOP)))
    assert items[-1] == (TOP, sum(RUNS) - 1, 1) and items[-4][0] == TOP - 1


def test_no_query_in_the_lattice_gives_no_items():
    outside, items = check(torch.full((5,), -1, dtype=torch.int64))
    assert outside == 5 and items == []


def test_cells_sort_stably_and_number_the_occupied_cells():
    g = torch.Generator().manual_seed(7)
    n = 2000
    keys = torch.randint(0, 40, (n,), generator=g, dtype=torch.int64) * (1 << 21)
    keys[::97] = TOP
    points = torch.rand(n, 3, generator=g, dtype=torch.float64)
    cells = cloud_lattice.Cells(points, keys)
    want = np.argsort(keys.numpy(), kind="stable")                              # equal keys keep the caller's order
    assert torch.equal(cells.order, torch.from_numpy(want))
    assert cells.index.dtype == torch.int32 and torch.equal(cells.index.to(torch.int64), cells.order)
    assert torch.equal(cells.sorted, points[cells.order]) and cells.sorted.is_contiguous()
    uniq, count = np.unique(keys.numpy(), return_counts=True)
    assert torch.equal(cells.ukeys, torch.from_numpy(uniq)) and int(cells.tstart[0]) == 0 and int(cells.tstart[-1]) == n
    assert torch.equal(cells.tstart[1:] - cells.tstart[:-1], torch.from_numpy(count))


def test_the_cloud_as_its_own_queries_is_cut_by_the_same_cutter():
    """cloud_filter.Search takes its items from Cells.items(); accuracy.nearest and register from work_items()."""
    keys = runs_of((3, 7, 8, 1 << 21, 1 << 42))
    shuffle = torch.randperm(keys.numel(), generator=torch.Generator().manual_seed(5))
    cells = cloud_lattice.Cells(torch.zeros(keys.numel(), 3, dtype=torch.float64), keys[shuffle])
    ks = torch.sort(keys[shuffle], stable=True)
    _, qorder, items = cloud_lattice.work_items(ks.values, ks.indices)
    assert torch.equal(qorder, cells.order)
    for a, b in zip(cells.items(), items):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert as_list(items) == loop_items(keys)[1]
