"""Shared by tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py: the board-symmetry rule written out once more on the
host (numpy), the host permutation of a packed record, and positions of the golden games."""
import os

import numpy as np

from go_replay import GAME_CONFIGS
from sayuri_amd.engine import Game, expand_packed, pack_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_GAMES = os.path.join(ROOT, "tests", "golden", "go_games.npz")
# games of tests/golden/go_games.npz on 19 / 13 / 9 boards with the 43-plane encoder
GAME_OF_SIZE = {19: 0, 13: 3, 9: 4}


def symm_index(bs: int, s: int) -> np.ndarray:
    """idx[d] = the source cell of output cell d = y*bs + x under symmetry s (include/sayuri_hip.h; reference
    src/game/symmetry.cc:97-123)."""
    y, x = np.divmod(np.arange(bs * bs), bs)
    tx, ty = (y, x) if s & 4 else (x, y)
    if s & 2:
        tx = bs - 1 - tx
    if s & 1:
        ty = bs - 1 - ty
    return ty * bs + tx


def permute_record(rec: np.ndarray, binary: int, bs: int, s: int) -> np.ndarray:
    """The record whose every plane shows, at cell d, cell symm_index(bs, s)[d] of `rec`'s."""
    planes = expand_packed(rec, binary, bs, binary + 6)
    return pack_planes(planes[:, symm_index(bs, s)], binary)


def golden_game_at(golden, gi: int, step: int) -> Game:
    """Game `gi` of the golden file after its first `step` recorded operations."""
    cfg = GAME_CONFIGS[gi]
    g = Game(cfg["board"], cfg["komi"], cfg["scoring"])
    if cfg["handicap"]:
        assert g.fixed_handicap(cfg["handicap"])
    for op, move in golden[f"g{gi}_moves"][:step]:
        if int(op) == 0:
            assert g.play(int(move))
        elif int(op) == 1:
            assert g.undo()
        else:
            g.set_territory_helper_from_ownership()
    return g
