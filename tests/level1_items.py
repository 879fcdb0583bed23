"""Random work items with what lowering level 1 folds planted in them (graph_framework_amd/csrc/merge.hpp and
asm_body.hpp, options.hpp `level`), for tests/test_level1.py on the CPU and tests/test_gpu_level1.py on the device.

tests/gfir_random.py hash-conses its records, so an item it builds has no two records of one node, and it multiplies by
-1.0 or gathers a negated table only by chance.  planted_item() grows such an item and keeps adding, between its records:

    * mul(-1.0, x) and mul(x, -1.0), of values, of gathers and of one another (a sign record of a sign record);
    * the twin of an add, a mul or an fma with the first two operands swapped;
    * a second record of a square root;
    * gathers of -1.0 times the table of an earlier gather, and of +0.5 and -0.5 times it, at the same cell.

The new records join the values the item goes on to use, so some end up as denominators, root arguments, gather
arguments, setters and outputs — where the fold must fall back to the multiplication — and most as operands of
arithmetic, where it applies.
"""
import numpy as np

import gfir_random
from gfir_random import ADD, FMA, GATHER1, GATHER2, MUL, SQRT


def planted_item(seed, num_inputs=6, num_nodes=400, num_outputs=3, num_setters=3, name="planted"):
    """Returns (GFIR bytes, {what was planted: how many})."""
    rng = np.random.default_rng(seed)
    b = gfir_random.Builder(rng, "f64", num_inputs)
    planted = {"sign": 0, "swapped": 0, "sqrt": 0, "flipped": 0, "halves": 0}

    def raw(record, bound):
        """A record of its own, whatever the builder already holds (no hash-consing)."""
        b.code.append(record)
        b.bound.append(float(bound))
        b.values.append(len(b.code) - 1)
        return len(b.code) - 1

    def multiple(table, factor):
        b.tables.append((np.float64(factor)*b.tables[table]).astype(np.float64))
        return len(b.tables) - 1

    zeros = (0.0, 0.0, 0.0, 0.0)
    while len(b.code) < num_nodes:
        b.grow()
        r = rng.random()
        if r < 0.10:
            x = b.pick()
            minus_one = b.constant(-1.0)
            first = raw((MUL, minus_one, x, gfir_random.NONE, 0, zeros) if rng.random() < 0.5 else
                        (MUL, x, minus_one, gfir_random.NONE, 0, zeros), b.bound[x])
            planted["sign"] += 1
            if rng.random() < 0.3:          # -(-x), and a twin of the first with the constant on the other side
                raw((MUL, minus_one, first, gfir_random.NONE, 0, zeros), b.bound[x])
                raw((MUL, x, minus_one, gfir_random.NONE, 0, zeros), b.bound[x])
                planted["sign"] += 2
        elif r < 0.18:
            recent = [k for k in range(max(0, len(b.code) - 60), len(b.code)) if b.code[k][0] in (ADD, MUL, FMA) and b.code[k][1] != b.code[k][2]]
            if recent:
                k = recent[int(rng.integers(0, len(recent)))]
                op, x, y, z, aux, imm = b.code[k]
                raw((op, y, x, z, aux, imm), b.bound[k])
                planted["swapped"] += 1
        elif r < 0.22:
            roots = [k for k in range(len(b.code)) if b.code[k][0] == SQRT]
            if roots:
                k = roots[int(rng.integers(0, len(roots)))]
                raw(b.code[k], b.bound[k])
                planted["sqrt"] += 1
        elif r < 0.32:
            gathers = [k for k in range(len(b.code)) if b.code[k][0] in (GATHER1, GATHER2)]
            if gathers:
                k = gathers[int(rng.integers(0, len(gathers)))]
                op, x, y, z, table, imm = b.code[k]
                if rng.random() < 0.5:
                    raw((op, x, y, z, multiple(table, -1.0), imm), b.bound[k])
                    planted["flipped"] += 1
                else:
                    raw((op, x, y, z, multiple(table, 0.5), imm), b.bound[k])
                    raw((op, x, y, z, multiple(table, -0.5), imm), b.bound[k])
                    planted["halves"] += 1
    tail = b.values[-max(32, num_outputs + num_setters):]
    outputs = [tail[int(rng.integers(0, len(tail)))] for _ in range(num_outputs)]
    setters = []
    for target in rng.permutation(num_inputs)[:num_setters]:
        v = tail[int(rng.integers(0, len(tail)))]
        if b.bound[v] > 1.0:
            v = b.squash(v)
        setters.append((v, int(target)))
    return gfir_random.serialize(b, outputs, setters, num_inputs, name), planted
