"""A restatement of the reference's VAR / STDDEV accumulator (functions-aggregate/src/variance.rs VarianceGroupsAccumulator, stddev.rs):
Welford's update per value, Chan's merge of (count, mean, m2) states, and the final values with their NULL rules.  The truth the
variance tests compare the device with; itself checked against exact rational arithmetic (tests/test_variance_restatement.py)."""
import math
from fractions import Fraction

FUNCS = ("var", "var_pop", "stddev", "stddev_pop")


def update(state, x):
    """variance.rs update: NULL arguments are skipped"""
    n, mean, m2 = state
    if x is None:
        return state
    n += 1
    d1 = x - mean
    mean = d1 / n + mean
    return n, mean, m2 + d1 * (x - mean)


def merge(a, b):
    """variance.rs merge: a partial state of count 0 is skipped"""
    (n1, mean1, m21), (n2, mean2, m22) = a, b
    if n2 == 0:
        return a
    if n1 == 0:
        return b
    n = n1 + n2
    d = mean1 - mean2
    return n, mean1 * n1 / n + mean2 * n2 / n, m21 + m22 + d * d * n1 * n2 / n


def state_of(values):
    s = (0, 0.0, 0.0)
    for x in values:
        s = update(s, x)
    return s


def finish(state, func):
    """VAR_SAMP / STDDEV_SAMP: NULL below two values; VAR_POP / STDDEV_POP: NULL without a value"""
    n, _, m2 = state
    sample = func in ("var", "stddev")
    if n <= (1 if sample else 0):
        return None
    v = m2 / (n - 1 if sample else n)
    return math.sqrt(v) if func.startswith("stddev") else v


def exact_variance(values, func):
    """the exact value over the Float64 inputs (as rationals), or None by the same NULL rules"""
    xs = [Fraction(x) for x in values if x is not None]
    n = len(xs)
    sample = func in ("var", "stddev")
    if n <= (1 if sample else 0):
        return None
    mean = sum(xs) / n
    v = sum((x - mean) ** 2 for x in xs) / (n - 1 if sample else n)
    return math.sqrt(v) if func.startswith("stddev") else float(v)
