"""Several playouts in flight inside one tree (option playouts_in_flight; csrc/engine/search.h) on the MI355X: a group
request has the bits of its requests sent one by one, a search has the same result whichever way its leaves travel, and
one tree is searched faster with eight playouts in flight than with one."""
import time

import numpy as np
import pytest

from _ensemble import GAME_OF_SIZE, GOLDEN_GAMES, golden_game_at
from _golden import Golden
from sayuri_amd import search as S
from sayuri_amd.engine import Game
from sayuri_amd.pipe import HipForwardPipe

pytestmark = pytest.mark.gpu

B = 19


def golden_positions():
    """Eleven positions of the golden games: four on 19x19 and 13x13, three on 9x9."""
    golden = np.load(GOLDEN_GAMES)
    out = []
    for bs, gi in GAME_OF_SIZE.items():
        n = len(golden[f"g{gi}_moves"])
        for step in (3, n // 3, (2 * n) // 3, n - 2)[:4 if bs > 9 else 3]:
            out.append((bs, golden_game_at(golden, gi, step)))
    assert len(out) == 11
    return out


# ------------------------------------------------------------------------------------------------- a. group bits
@pytest.mark.parametrize("latency", [True, False], ids=["latency", "default"])
def test_a_group_has_the_bits_of_its_requests_alone(tmp_weights_dir, latency):
    g = Golden("net_20b256", tmp_weights_dir)
    pipe = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, latency=latency)
    try:
        assert pipe.AcceptsGroup()
        cases = [(game.planes(0, 4), bs) for bs, game in golden_positions()]
        before = pipe.pump_times()
        got = pipe.ForwardGroup(cases)
        after = pipe.pump_times()
        assert after["batches"] - before["batches"] == 1 and after["evals"] - before["evals"] == 11
        for i, ((planes, bs), out) in enumerate(zip(cases, got)):
            want = pipe.ForwardPacked([planes], [bs])[0]
            n = bs * bs
            for name, a, b in [("probabilities", out[:n], want[:n]), ("ownership", out[n:2 * n], want[n:2 * n])] + \
                              [(f"scalar {k}", out[2 * n + k:2 * n + k + 1], want[2 * n + k:2 * n + k + 1]) for k in range(9)]:
                assert np.array_equal(a, b), (i, bs, name)
        assert len({o.tobytes() for o in got}) == 11, "positions whose outputs coincide check nothing"
    finally:
        pipe.Destroy()


# ------------------------------------------------------------------------------------------------- b. search bits
def search_once(pipe, no_cache, grouped, flight=8):
    net = S.Network(pipe=pipe, options=dict(no_cache=no_cache, group_forward=grouped))
    game = Game(9, 7.0)
    search = S.Search(game, net, dict(playouts=200, playouts_in_flight=flight), seeds=(3, 4))
    before = pipe.pump_times()
    res = search.computation(200)
    after = pipe.pump_times()
    stats = search.flight_stats()
    assert res["playouts"] == 200 and stats["in_flight"] == 0
    assert after["evals"] - before["evals"] == net.queries()
    search.close()
    net.close()
    return res, stats, after["batches"] - before["batches"]


@pytest.mark.parametrize("no_cache", [0, 1], ids=["cache", "no_cache"])
def test_a_search_does_not_depend_on_how_its_leaves_travel(tmp_weights_dir, no_cache):
    """net_6b96, 9x9, K = 8, 200 playouts: as groups and one by one the search is the same (a position's bits do not depend
    on the batch it travels in), and a second run with the same seeds repeats it."""
    g = Golden("net_6b96", tmp_weights_dir)
    pipe = HipForwardPipe(g.weights_path, board_size=9, batch_size=16, fp16=True, waittime_ms=0)
    try:
        a, st_a, batches_a = search_once(pipe, no_cache, 1)
        b, st_b, batches_b = search_once(pipe, no_cache, 0)
        c, st_c, _ = search_once(pipe, no_cache, 1)
        for other, st in ((b, st_b), (c, st_c)):
            assert a.keys() == other.keys() and st == st_a
            for k in a:
                assert np.array_equal(a[k], other[k]), k
        assert st_a["leaves"] / st_a["rounds"] >= 2.0 and batches_a < batches_b / 2, (st_a, batches_a, batches_b)
    finally:
        pipe.Destroy()


# ------------------------------------------------------------------------------------------------- c. faster
def test_eight_playouts_in_flight_search_one_tree_faster(tmp_weights_dir, capsys):
    """net_20b256 on a latency pipe, one 19x19 mid-game position, cache off, 400 playouts: K = 1 (the search as it always
    was) against K = 8, interleaved, medians of 3 rounds of playouts per second.  The floor of 1.5 is reasoned, not measured:
    by profiles/r07_latency_small_batch.json one board makes the round trip in 0.657 ms and eight in 0.766 ms, 0.096 ms per
    leaf; even if the host spent as long per playout as a whole single round trip (0.66 ms, three times the encoder's worst
    case), the ratio would be (0.66 + 0.66) / (0.66 + 0.10) = 1.7.  A search that still sends batches of one has ratio 1.
    Measured on an MI355X (this test's own run): K = 1 1 582 playouts/s, K = 8 8 179, ratio 5.17, 6.88 leaves
    per round, no collisions."""
    g = Golden("net_20b256", tmp_weights_dir)
    game = golden_game_at(np.load(GOLDEN_GAMES), GAME_OF_SIZE[19], 120)
    pipe = HipForwardPipe(g.weights_path, board_size=B, batch_size=16, fp16=True, waittime_ms=0, latency=True)
    try:
        net = S.Network(pipe=pipe, options=dict(no_cache=True))
        rate = {1: [], 8: []}
        stats = {}
        for rnd in range(-1, 3):  # round -1: the warm-up
            for flight in rate:
                search = S.Search(game, net, dict(playouts=400, playouts_in_flight=flight), seeds=(5, 6))
                t0 = time.perf_counter()
                res = search.computation(100 if rnd < 0 else 400)
                took = time.perf_counter() - t0
                if rnd >= 0:
                    assert res["playouts"] == 400
                    rate[flight].append(res["playouts"] / took)
                    stats[flight] = search.flight_stats()
                search.close()
        one, eight = float(np.median(rate[1])), float(np.median(rate[8]))
        with capsys.disabled():
            print(f"\n[tree batch] net_20b256 latency pipe, one 19x19 position, 400 playouts, playouts/s: K=1 {one:.0f}, K=8 {eight:.0f}, "
                  f"ratio {eight / one:.2f}; K=8 leaves per round {stats[8]['leaves'] / stats[8]['rounds']:.2f}, collisions {stats[8]['collisions']}")
        assert eight >= 1.5 * one, (one, eight)
        net.close()
    finally:
        pipe.Destroy()
