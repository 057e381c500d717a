"""Cases shared by test_joint_groups_host.py (CPU) and test_joint_groups_gpu.py:
the conditional space of the group tests, and the slots, seed, rounds and
candidate counts of the batched joint round.  The host test checks through the
fp64 draw port that this seed excludes no draw and leaves every cell's winner
a clear margin under each slot's own pick stream, so no cell is skipped on
the GPU."""
import numpy as np

from hyperopt_amd import hp
from oracle import draw_oracle as D
from tests import joint_cases as JC
from tests.joint_reference import JOINT_STREAM

# -- the conditional space -------------------------------------------------------
# x, ly: unconditional dense; c option 0: a, b dense, qa quantized, the nested
# choice `inner` whose option 1 holds d1, d2; c option 1: e alone; sh is shared
# by options 0 and 1 of the choice k


def space():
    sh = hp.uniform('sh', 0, 1)
    return {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2),
            'c': hp.choice('c', [
                {'a': hp.uniform('a', -2, 2), 'b': hp.normal('b', 0, 1), 'qa': hp.quniform('qa', 0, 10, 2),
                 'inner': hp.choice('inner', [1.5, {'d1': hp.uniform('d1', 0, 4),
                                                    'd2': hp.lognormal('d2', 0, 1)}])},
                {'e': hp.uniform('e', 0, 1)}]),
            'k': hp.choice('k', [{'v': sh}, {'w': sh}, 0.25])}


def _sig(*paths):
    return frozenset(frozenset(p) for p in paths)


UNCONDITIONAL = _sig(())
SIGNATURES = {
    'x': UNCONDITIONAL, 'ly': UNCONDITIONAL, 'c': UNCONDITIONAL, 'k': UNCONDITIONAL,
    'a': _sig([('c', 0)]), 'b': _sig([('c', 0)]), 'qa': _sig([('c', 0)]), 'inner': _sig([('c', 0)]),
    'd1': _sig([('c', 0), ('inner', 1)]), 'd2': _sig([('c', 0), ('inner', 1)]),
    'e': _sig([('c', 1)]),
    'sh': _sig([('k', 0)], [('k', 1)]),
}
GROUPS = [(0, ['ly', 'x']), (1, ['a', 'b']), (2, ['d1', 'd2'])]


def loss(d):
    """Couples the two labels inside each branch (a with b, d1 with d2)."""
    out = 0.05 * d['x'] ** 2 + 0.05 * np.log(d['ly']) ** 2
    c = d['c']
    if 'a' in c:
        out += (c['a'] - c['b']) ** 2 + 0.1 * (c['a'] + c['b'] - 1.0) ** 2 + 0.01 * c['qa']
        if isinstance(c['inner'], dict):
            out += (c['inner']['d1'] - 2.0 * np.log(c['inner']['d2']) - 1.0) ** 2
        else:
            out += 0.5
    else:
        out += 0.8 + c['e']
    return float(out)


# -- the batched round -------------------------------------------------------------
SLOTS = ['d2', 'd20', 'd33', 'd70']           # JC.GROUPS names: slot j holds SLOTS[j]
SEED = 31
ROUNDS = [0, 7, 4294967295, 7, 3, 1, 2, 9, 8, 6, 5]
COUNTS = [24, 1, 65, 300]
DRAW_SLOT = 2                                 # the slot of the draw check (j > 0)

FUSED = ('d5_k300', 77, 24, 5500)             # group, seed, n_candidates, rounds 0 .. 5499
TIE_ROUNDS = list(range(11))
TIE_COUNTS = [1, 24, 5000]


def pick_stream(slot):
    return JOINT_STREAM - slot


def port_draw(ref, seed, rnd, g, stream):
    """JointRef.port_draw with the component pick on `stream`: (component [n],
    values [n, D], excluded [n]) of candidates g by the fp64 draw port."""
    g = np.asarray(g, dtype=np.uint64)
    pf = ref.pick_fold()
    wp, wu = D.draw_words(seed, stream, rnd, g)
    comp = D.pick(pf, wp)
    excl = D.excluded(pf, wp, wu)
    vals = np.empty((len(g), ref.D))
    for d, dim in enumerate(ref.dims):
        wpd, wud = D.draw_words(seed, dim.stream, rnd, g)
        for k in np.unique(comp):
            sel = comp == k
            f = ref.fold(int(k), d)
            _, _, x, v = D.draw_fp64(f, wpd[sel], wud[sel])
            vals[sel, d] = v
            excl[sel] |= D.excluded(f, wpd[sel], wud[sel], x)
    return comp, vals, excl


def set_slots(eng, names=SLOTS):
    """Clear the engine's joint slots and put JC.group(names[j]) in slot j
    with the pick stream TPE_JOINT_STREAM - j; returns the JointRefs."""
    eng.clear_joint_groups()
    refs = [JC.group(name) for name in names]
    for j, ref in enumerate(refs):
        eng.set_joint_group(j, pick_stream(j), *JC.engine_args(ref))
    return refs
