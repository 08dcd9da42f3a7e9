"""Plain-Python model of the gate satisfiability check (boojum_amd.gates.check_if_satisfied,
bj_gate_set_satisfied_d): CSReferenceAssembly::check_if_satisfied
(cs/implementations/satisfiability_test.rs:15-353) said over captured programs.

Term k of row r is unsatisfied iff selector_g(r) * term_k(r) != 0 mod p, k being the running term
index of the challenges (terms, then repetitions, then gates, segments carrying it on).  The loops
are the definition's: rows, then gates, repetitions and terms, so the first failure met is the
first in (row, k) order.  Column cells may be any u64 word; they are reduced on the way in."""
import gates_model as M

P = M.P
NO_KEY = (1 << 64) - 1


def row_terms(placements, variables, witnesses, constants):
    """[(k, selector, term)] of one row given as three lists of integers."""
    v, w, c = ([int(x) % P for x in col] for col in (variables, witnesses, constants))
    out, k = [], 0
    for pl in placements:
        sel = M.selector_at(pl.selector_path, c)
        bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
        for rep in range(pl.num_repetitions):
            off = tuple(b + rep * p for b, p in zip(bases, per))
            for term in M.interpret(pl.program, v, w, c, off):
                out.append((k, sel, term))
                k += 1
    return out


def check(placements, variables, witnesses, constants, rows=None):
    """variables, witnesses, constants: (C, n) arrays (or lists of columns; an empty list for a kind
    the set never names).  Returns (count, first): the number of unsatisfied (row, term) pairs in
    the window and the first of them as (row, k, value), or None."""
    n = len((variables if len(variables) else constants if len(constants) else witnesses)[0])
    begin, count = (0, n) if rows is None else rows
    assert 0 <= begin and count >= 1 and begin + count <= n
    failures, first = 0, None
    for r in range(begin, begin + count):
        row = [[int(col[r]) for col in cols] for cols in (variables, witnesses, constants)]
        for k, sel, term in row_terms(placements, *row):
            if sel * term % P:
                failures += 1
                if first is None:
                    first = (r, k, term)
    return failures, first


def status_record(placements, variables, witnesses, constants, rows=None):
    """The 4 words bj_gate_set_satisfied_d leaves after every segment of the set."""
    failures, first = check(placements, variables, witnesses, constants, rows)
    if first is None:
        return [0, NO_KEY, 0, 0]
    return [failures, first[0] << 32 | first[1], first[2], 0]


def locate_brute(placements, k):
    """(gate, subinstance, term) of the running term index k by enumeration."""
    i = 0
    for g, pl in enumerate(placements):
        for rep in range(pl.num_repetitions):
            for t in range(pl.program.num_quotient_terms):
                if i == k:
                    return g, rep, t
                i += 1
    raise IndexError(k)
