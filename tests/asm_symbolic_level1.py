"""Symbolic replay of a LEVEL-1 assembly statement (graph_framework_amd/csrc/asm_body.hpp, options.hpp `level`).

tests/asm_symbolic.py replays a statement and holds every definition against the item's DAG, expression by expression.
At level 1 the statement folds what is equal for every operand that is not a NaN: a mul by -1.0
and a gather of a table derived by the factor -1.0 write no instruction — their uses carry a `neg` modifier — and
records that differ only in the order of the operands of add, mul or fma's product are computed once.  This module runs
the same replay with BOTH sides normalised:

    mul(+-1.0, x)  <->  +-x
    mul(x, -k)     <->  -mul(x, k)          (a table value -k*p read from the register that holds k*p: `; twin` lines)
    add(x, y), mul(x, y), fma(x, y, z): x and y in one fixed order

and adds what the level-0 replay has no need for: every `; alias rJ = [-]name` line of the statement (a merged record,
a folded sign record, a folded gather) is held against the DAG too, so an alias that names the wrong record fails even
if no instruction reads it wrongly.
"""
import re

import asm_symbolic
from asm_symbolic import OPS, ReplayError, bits, statement_of  # noqa: F401  (re-exported for the tests)

ONE, MINUS_ONE = bits(1.0), bits(-1.0)
NOT_SIGN, INFINITY = (1 << 63) - 1, 0x7ff << 52
TWIN = re.compile(r"twin (c\d+_\d+) = (c\d+_\d+) \* (\d+)")
FOLDED_GATHER = re.compile(r"alias r(\d+) = -(c\d+_\d+)")
ALIAS = re.compile(r"alias r(\d+) = (-?)([rc][\d_]+)")


class Expressions(asm_symbolic.Expressions):
    """Hash-consed expressions, normalised as the module's text says."""

    def mk(self, *key):
        if key[0] == "mul":
            for x, k in ((key[1], key[2]), (key[2], key[1])):
                constant = self.keys[k]
                if constant[0] == "const" and constant[1] in (ONE, MINUS_ONE):
                    return x if constant[1] == ONE else self.neg(x)
            for x, k in ((key[1], key[2]), (key[2], key[1])):
                constant = self.keys[k]
                if constant[0] == "const" and constant[1] >> 63 and (constant[1] & NOT_SIGN) <= INFINITY:
                    return self.neg(self.mk("mul", x, self.const(constant[1] & NOT_SIGN)))
        if key[0] in ("add", "mul", "fma") and key[2] < key[1]:
            key = (key[0], key[2], key[1]) + tuple(key[3:])
        return super().mk(*key)


def replay(blob, source):
    """asm_symbolic.replay() for a level-1 statement; returns its statistics plus the aliases checked."""
    lines = statement_of(source)
    folded_gathers = {}
    for line in lines:
        m = FOLDED_GATHER.fullmatch(line.partition(";")[2].strip()) if not line.partition(";")[0].strip() else None
        if m:
            folded_gathers[int(m.group(1))] = m.group(2)
#  Records the statement names after an earlier record (`alias rJ = rI`: merged, at level 0 or 1).  The piece handed in is
#  the level-0 form, in which a quotient may still name a denominator J that level 1 merged into I: the statement then
#  defines the reciprocal q<I>.  The replay keeps its books of tracked denominators by those names, so denominators are
#  renamed here — to the same expression if the alias is right, which the check at the end establishes for every alias.
    renamed = {}
    for line in lines:
        m = ALIAS.fullmatch(line.partition(";")[2].strip()) if not line.partition(";")[0].strip() else None
        if m and m.group(3)[0] == "r" and int(m.group(3)[1:]) >= int(m.group(1)):
            raise ReplayError("r%s is named after a record that is not an earlier one\n    in: %s" % (m.group(1), line))
        if m and not m.group(2) and m.group(3)[0] == "r":
            renamed[int(m.group(1))] = int(m.group(3)[1:])

    def parse(data):
        item = dict(asm_symbolic_parse(data))
        ins = item["ins"].copy()
        for k in range(len(ins)):
            if int(ins["op"][k]) == OPS["DIV"]:
                b = int(ins["b"][k])
                while b in renamed:
                    b = renamed[b]
                ins["b"][k] = b
        item["ins"] = ins
        return item

#  Table values the statement reads from their twin's register and may never make: what they are, as a `def` line says it.
    twins = {}
    for line in lines:
        m = TWIN.fullmatch(line.partition(";")[2].strip()) if not line.partition(";")[0].strip() else None
        if m:
            twins[m.group(1)] = (m.group(2), int(m.group(3)))
    made = []

    class Expected(asm_symbolic.Expected):
        def __init__(self, item, ex):
            super().__init__(item, ex)
            made.append(self)

        def node(self, i):
            if i in folded_gathers and i not in self.memo:
#  the gather of a table that is -1.0 times its parent (the writer's own statement about the tables, as at level 0)
                self.memo[i] = self.ex.mk("mul", self.cells[folded_gathers[i]], self.ex.const(MINUS_ONE))
            name = self.alias.get(i)
            if name in twins and i not in self.memo:
                self.cells[name] = self.ex.mk("mul", self.cells[twins[name][0]], self.ex.const(twins[name][1]))
            return super().node(i)

    saved = asm_symbolic.Expressions, asm_symbolic.Expected, asm_symbolic.parse
    asm_symbolic_parse = saved[2]
    asm_symbolic.Expressions, asm_symbolic.Expected, asm_symbolic.parse = Expressions, Expected, parse
    try:
        stats = asm_symbolic.replay(blob, source)
    finally:
        asm_symbolic.Expressions, asm_symbolic.Expected, asm_symbolic.parse = saved
    expected = made[0]
    ex = expected.ex
    checked = 0
    for line in lines:
        text, _, note = line.partition(";")
        m = ALIAS.fullmatch(note.strip()) if not text.strip() else None
        if not m:
            continue
        record, minus, name = int(m.group(1)), m.group(2) == "-", m.group(3)
        if name[0] == "r":
            value = expected.node(int(name[1:]))
        else:
            value = expected.cells.get(name)
            if value is None and record in folded_gathers:
                continue            # (a gather nothing reads: its parent's value was never brought in)
            if value is None:
                raise ReplayError("alias of r%d names %s, which the statement never loads\n    in: %s" % (record, name, line))
        if minus:
            value = ex.neg(value)
        want = expected.node(record)
        if want != value:
            raise ReplayError("r%d is named %s%s = %s, the item says %s\n    in: %s"
                              % (record, m.group(2), name, ex.show(value), ex.show(want), line))
        checked += 1
    stats["aliases"] = checked
    stats["folded_gathers"] = len(folded_gathers)
    stats["twins"] = len(twins)
    return stats
