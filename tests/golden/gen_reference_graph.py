"""The reference's pyll graph of one search space, as data.

Needs a source tree of the reference hyperopt:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_reference_graph.py <reference tree>

Builds the space of tests/test_api.py::test_compile_reference_domain with the
reference's own hp.* constructors, takes the reference Domain's `expr` and
records every node reachable from it: its operator `name`, its positional
and named arguments (as node numbers; node 0 is the root, a node shared by
several parents is recorded once) and, for a literal, its `obj`.  Stored as
tests/golden/reference_domain_graph.json -- data only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
sys.path[:0] = [os.path.join(REPO, 'tools', 'refshim'), sys.argv[1]]

from hyperopt import hp  # noqa: E402  (reference)
from hyperopt.base import Domain  # noqa: E402


def space():
    return {'a': hp.choice('a', [{'u': hp.uniform('u', 0, 1)}, {'v': hp.qloguniform('v', 0, 3, 2)}]),
            'k': hp.pchoice('k', [(.1, 0), (.9, 1)]), 'n': hp.qnormal('n', 0, 10, 2)}


def record(expr):
    number, nodes, stack = {id(expr): 0}, [None], [expr]
    keep = [expr]                       # (ids stay unique while the nodes live)

    def num(n):
        if id(n) not in number:
            number[id(n)] = len(nodes)
            nodes.append(None)
            stack.append(n)
            keep.append(n)
        return number[id(n)]
    while stack:
        n = stack.pop()
        rec = {'name': n.name, 'pos_args': [num(a) for a in n.pos_args],
               'named_args': [[k, num(v)] for k, v in n.named_args]}
        if n.name == 'literal':
            obj = n.obj
            if not (obj is None or isinstance(obj, (bool, int, float, str))):
                raise TypeError('literal %r is not plain data' % (obj,))
            rec['obj'] = obj
        nodes[number[id(n)]] = rec
    return nodes


def main():
    nodes = record(Domain(lambda x: 0, space()).expr)
    with open(os.path.join(HERE, 'reference_domain_graph.json'), 'w') as f:
        json.dump({'note': 'the reference Domain.expr of the space in gen_reference_graph.py: '
                           'per node its operator name, argument node numbers and literal obj',
                   'root': 0, 'nodes': nodes}, f, indent=1)
        f.write('\n')
    print(len(nodes), 'nodes')


if __name__ == '__main__':
    main()
