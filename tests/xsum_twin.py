"""Python twin of the lane moves under the wave reductions of csrc/csmp_kernels.hpp, on SYMBOLS: xs32 / xs16 (v_permlane32_swap /
v_permlane16_swap on two inputs, then one addition), the four in-row steps of row_xsum, wave_xsum, and the set reductions of the shared
sweep (sweep_body_multi: a set of four, a set of two).

A wave is a list of 64 expressions, one per lane.  A leaf is (input, lane); an addition is the frozenset of its two operands: the
additions are commutative, so the order inside a pair does not matter, but which pairs are added, and in which order of steps, does --
two expressions are equal exactly when they are the same tree of unordered pairs, which is what makes the Float64 results bit-equal.

set_slots(R) is the written-down assignment of (member, column of the pair) to the slots of the sets (the comment above
sweep_body_multi): tests/test_multi_epilogue_static.py pins it and reads the same order out of the kernel's source."""
WAVE = 64


def leaves(name):
    """the 64 lanes of an input"""
    return [(name, lane) for lane in range(WAVE)]


def add(a, b):
    assert a != b
    return frozenset((a, b))


def permlane32_swap(x, y):
    """X' = [X_lo | Y_lo], Y' = [X_hi | Y_hi]: the upper half of x and the lower half of y change places"""
    return x[:32] + y[:32], x[32:] + y[32:]


def permlane16_swap(x, y):
    """the odd rows of x and the even rows of y change places: X' = rows [X0, Y0, X2, Y2], Y' = rows [X1, Y1, X3, Y3]"""
    row = lambda v, q: v[16 * q:16 * q + 16]
    return row(x, 0) + row(y, 0) + row(x, 2) + row(y, 2), row(x, 1) + row(y, 1) + row(x, 3) + row(y, 3)


def xs32(x, y):
    a, b = permlane32_swap(x, y)
    return [add(a[l], b[l]) for l in range(WAVE)]


def xs16(x, y):
    a, b = permlane16_swap(x, y)
    return [add(a[l], b[l]) for l in range(WAVE)]


def row_xsum(v):
    """xor 8 (row_ror:8), xor 4 (row_shl:4 / row_shr:4 under bank masks), xor 2 and xor 1 (quad permutations): all inside a row of 16"""
    for s in (8, 4, 2, 1):
        v = [add(v[l], v[(l & ~15) | ((l & 15) ^ s)]) for l in range(WAVE)]
    return v


def wave_xsum(v):
    v = xs32(v, v)
    v = xs16(v, v)
    return row_xsum(v)


def set_of_four(v0, v1, v2, v3):
    """slot q ends in lane row q"""
    return row_xsum(xs16(xs32(v0, v2), xs32(v1, v3)))


def set_of_two(v0, v1):
    """slot q ends in the wave's half q"""
    v = xs32(v0, v1)
    return row_xsum(xs16(v, v))


def inputs_of(expr):
    """the names of the inputs an expression holds anything of"""
    if isinstance(expr, frozenset):
        return set().union(*(inputs_of(e) for e in expr))
    return {expr[0]}


def set_slots(R):
    """the sets of a group of R members, each a list of its slots' (member, column of the pair): sets of four first, then the set of
    two of an odd R"""
    sets = [[(2 * s + m, j) for m in (0, 1) for j in (0, 1)] for s in range(R // 2)]
    if R & 1:
        sets.append([(R - 1, 0), (R - 1, 1)])
    return sets


def lane_slot(nslots, lane):
    """the slot of a set of `nslots` whose total lane `lane` receives"""
    return lane >> 4 if nslots == 4 else lane >> 5
