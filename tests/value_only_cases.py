"""Shapes and the cell check of tests/test_value_only_edges_gpu.py (no GPU
here: tests/test_value_only_edges_host.py runs both).

A packed-map call of n_rounds x C candidates takes k_pick_win -- the only
kernel that decides a (round, label) cell from the screen's bounds alone --
from kWinMinN = 8192 candidate slots per label on; below that it takes
k_pick_packed, which decides nothing.  The packed map itself ends at
C = kTile - 1 = 1023 candidates per round (round_args: `n < kTile`); a call
of C = 1024 runs the tile map, one round per grid.z.

check_cells holds a value-only round's winners to the exact scores of the
round's own candidates (tests/bx_reference.py, long double).
"""
import numpy as np

K_WIN_MIN_N = 8192        # tpe_engine.hip kWinMinN
K_BLOCK = 256             # tpe_ctx.h kBlock: rounds per workgroup of k_pick_win
K_BX_R = 4                # tpe_engine.hip kBxR: candidates per thread of the packed expansion screen
K_TILE = 1024             # tpe_engine.hip kTile: the packed map holds C < kTile
K_VALUE_MARGIN = 1e-9     # tpe_engine.hip kValueMargin

C_DEFAULT = 24
N_ROUNDS = 352
BIG_IDS = (7 + 2 ** 20, 2 ** 31 - 1)
COUNTS = [1, 2, 33, 256, 257, 1024]
N_BELOW_THRESHOLD = 341   # x 24 = 8184 slots: one round short of kWinMinN
# over_unclipped (16386 above components): the independent check covers
# these rounds only -- the first 64 and the two large ids
N_CHECKED_OVER_UNCLIPPED = 64

WINNER_BAR = 1e-9                    # max(s) - s[winner], test_bx_index_gpu.py's bar for a round's winner
DECIDED_GAP = 0.5 * K_VALUE_MARGIN   # a decided winner's exact lead, relative to max(1, |s[winner]|)
MAX_SKIPPED = 0.01                   # share of a (case, label)'s cells left out (a non-finite exact score)


def default_ids(n_rounds=N_ROUNDS):
    """0 .. n_rounds - 1 with the last two replaced by a large id and the
    largest id a trial can carry."""
    ids = list(range(n_rounds))
    ids[-2:] = BIG_IDS
    return ids


def rounds_for(C):
    """ceil(8192 / C) + 3 rounds: just past kWinMinN slots."""
    return (K_WIN_MIN_N + C - 1) // C + 3


def check_cells(s, index, decided):
    """s [R, C]: the exact scores of each round's candidates (any float
    type); index [R]: the reported winner; decided [R]: the cell was settled
    from the bounds alone.  Returns (skipped [R] bool, failures): a cell with
    a candidate whose exact score is not finite is skipped; every other cell's
    winner is within WINNER_BAR of the best exact score, and a decided cell's
    winner is the strict exact argmax with a lead of at least DECIDED_GAP x
    max(1, |s[winner]|) (a round of one candidate: its second is -inf).
    failures: (round position, what, winner, its score, rival, its score)."""
    s = np.asarray(s)
    R, C = s.shape
    index = np.asarray(index, dtype=np.int64)
    decided = np.asarray(decided, dtype=bool)
    skipped = ~np.all(np.isfinite(s), axis=1)
    fails = []
    for r in np.where(~skipped)[0]:
        w = int(index[r])
        if not 0 <= w < C:
            fails.append((int(r), 'index out of range', w, float('nan'), -1, float('nan')))
            continue
        row = s[r]
        best = int(np.argmax(row))
        if float(row[best] - row[w]) > WINNER_BAR:
            fails.append((int(r), 'winner below the exact best', w, float(row[w]), best, float(row[best])))
            continue
        if decided[r] and C > 1:
            others = np.delete(row, w)
            k = int(np.argmax(others))
            rival = k + (k >= w)
            lead = float(row[w] - others[k])
            if not lead >= DECIDED_GAP * max(1.0, abs(float(row[w]))):   # (a tie or a loss: lead <= 0)
                fails.append((int(r), 'decided without the exact lead', w, float(row[w]), rival, float(row[rival])))
    return skipped, fails
