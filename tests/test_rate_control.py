"""aivc_amd.rate_control.search_rates on tables of sizes (no device, no torch): the search is DEFINED step by step (its docstring),
so every case is compared with a line-by-line replay of that definition written here, and with what the definition implies
(the chosen rate fits, its neighbour toward the rich end does not, where the table is monotone)."""
import math

import pytest

from aivc_amd import rate_control as rc


def table_probe(tables, grid, calls):
    """probe over tables[u][grid position]; every call is recorded as its list of (unit, rate) pairs"""
    pos = {r: i for i, r in enumerate(grid)}

    def probe(pairs):
        calls.append(list(pairs))
        return [tables[u][pos[r]] for u, r in pairs]
    return probe


def replay(table, grid, budget):
    """the definition, for one unit -> (rate, bytes, over_budget, [(rate, bytes) in the order priced])"""
    trace = [(grid[0], table[0])]
    if len(grid) == 1:
        return grid[0], table[0], table[0] > budget, trace
    trace.append((grid[-1], table[-1]))
    top = len(grid) - 1
    lean_is_last = table[-1] < table[0]  # fewer bytes; a tie: grid[0]
    at = (lambda p: top - p) if lean_is_last else (lambda p: p)  # position counted from the lean end -> grid position
    lean, rich = table[at(0)], table[at(top)]
    if rich <= budget:
        return grid[at(top)], rich, False, trace
    if lean > budget:
        return grid[at(0)], lean, True, trace
    lo, hi = 0, top
    while hi - lo != 1:
        mid = (lo + hi) // 2
        trace.append((grid[at(mid)], table[at(mid)]))
        if table[at(mid)] <= budget:
            lo = mid
        else:
            hi = mid
    return grid[at(lo)], table[at(lo)], False, trace


def run(tables, grid, budgets):
    calls = []
    got = rc.search_rates(table_probe(tables, grid, calls), len(tables), grid, budgets)
    assert len(calls) <= rc.max_probe_calls(len(grid))
    assert rc.max_probe_calls(len(grid)) == (1 if len(grid) == 1 else 2 + math.ceil(math.log2(len(grid) - 1)))
    for pairs in calls:
        assert all(r in grid for _, r in pairs)
        assert len({u for u, _ in pairs}) == len(pairs)  # a call prices a unit once
    for u, ch in enumerate(got):
        want = replay(tables[u], grid, budgets[u])
        assert (ch.rate, ch.nbytes, ch.over_budget, list(ch.probes)) == want, 'unit %d' % u
    return got, calls


GRID = rc.rate_grid(3)  # 0, 1/16, ..., 2: 33 points


def test_grid():
    assert GRID == [i / 16 for i in range(33)]
    assert rc.rate_grid(3, 0.5) == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert rc.rate_grid(1) == [0.0]
    for bad in (0.1, 0.0, -0.0625):
        with pytest.raises(ValueError):
            rc.rate_grid(3, bad)
    with pytest.raises(ValueError):
        rc.rate_grid(3, 0.75)  # does not end on nb_rates - 1


def test_sizes_rising_with_the_index():
    table = [100 + 10 * i for i in range(33)]
    (ch,), calls = run([table], GRID, [255])
    assert ch.rate == 15 / 16 and ch.nbytes == 250 and not ch.over_budget
    assert len(calls) == 2 + 5
    assert calls[0] == [(0, 0.0)] and calls[1] == [(0, 2.0)]


def test_sizes_falling_with_the_index():
    table = [100 + 10 * (32 - i) for i in range(33)]  # the rich end is index 0
    (ch,), _ = run([table], GRID, [255])
    assert ch.rate == 17 / 16 and ch.nbytes == 250 and not ch.over_budget
    assert table[GRID.index(ch.rate) - 1] > 255  # the neighbour toward the rich end


def test_non_monotone_table_is_the_replay_of_the_definition():
    table = [100, 180, 120, 300, 140, 260, 150, 400, 90, 500, 130, 620, 170, 210, 640, 230, 700]
    grid = rc.rate_grid(3, 0.125)
    assert len(grid) == len(table)
    for budget in (95, 100, 150, 200, 260, 450, 650, 699, 700):
        run([table], grid, [budget])  # (the comparison with replay() is in run)


def test_budget_equal_to_a_size_fits():
    table = [100 + 10 * i for i in range(33)]
    (ch,), _ = run([table], GRID, [250])
    assert ch.rate == 15 / 16 and ch.nbytes == 250 and not ch.over_budget


def test_rich_end_fits():
    table = [100 + 10 * i for i in range(33)]
    (ch,), calls = run([table], GRID, [420])
    assert ch.rate == 2.0 and ch.nbytes == 420 and not ch.over_budget and len(calls) == 2
    (ch,), calls = run([table[::-1]], GRID, [1000])
    assert ch.rate == 0.0 and ch.nbytes == 420 and len(calls) == 2


def test_lean_end_too_big():
    table = [100 + 10 * i for i in range(33)]
    (ch,), calls = run([table], GRID, [99])
    assert ch.rate == 0.0 and ch.nbytes == 100 and ch.over_budget and len(calls) == 2
    (ch,), _ = run([table[::-1]], GRID, [99])
    assert ch.rate == 2.0 and ch.over_budget


def test_one_and_two_point_grids():
    (ch,), calls = run([[123]], [0.0], [200])
    assert (ch.rate, ch.nbytes, ch.over_budget) == (0.0, 123, False) and len(calls) == 1
    (ch,), calls = run([[123]], [0.0], [100])
    assert ch.over_budget and len(calls) == 1
    (ch,), calls = run([[100, 200]], [0.0, 1.0], [150])
    assert (ch.rate, ch.nbytes, ch.over_budget) == (0.0, 100, False) and len(calls) == 2


def test_three_units_three_answers_and_each_alone():
    tables = [[100 + 10 * i for i in range(33)],          # rising
              [90 + 7 * (32 - i) for i in range(33)],     # falling
              [300 + i for i in range(33)]]               # the lean end is already too big
    budgets = [255, 200, 250]
    got, calls = run(tables, GRID, budgets)
    assert len({ch.rate for ch in got}) == 3 and got[2].over_budget and not got[0].over_budget
    # a round is one call with every open unit: never more pairs than units, and the first two calls hold them all
    assert [len(c) for c in calls[:2]] == [3, 3] and all(len(c) <= 2 for c in calls[2:])
    for u in range(3):
        (alone,), _ = run([tables[u]], GRID, [budgets[u]])
        assert alone == got[u]


def test_budgets_from_target_bpp():
    # 8 frames of 64 x 48 in units of 3: the last unit has 2 real frames, its padding repeat does not count
    assert rc.unit_budgets(0.43, 64, 48, 8, 3) == [495, 495, 330]
    assert rc.unit_budgets(0.43, 64, 48, 8, 3)[2] == math.floor(0.43 * 64 * 48 * 2 / 8)
    assert rc.unit_budgets(1.0, 16, 16, 3, 3) == [96]
    assert rc.unit_budgets(0.5, 17, 9, 4, 4) == [math.floor(0.5 * 17 * 9 * 4 / 8)]
