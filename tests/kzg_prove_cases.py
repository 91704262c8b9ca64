"""Test helper for KZG batch proving (vc_kzg_prove_many): every expected value is the oracle's.
protocol.KZG.quotient gives q and y; the expected proof is BN254.mul(g, sum_j c_j q_j mod r) with
c = kzg_lagrange_scalars(N, 100) -- the group element prove_point's MSM over the points c_j G gives,
at one scalar multiplication per opening instead of N (tests/test_kzg_prove_many_host.py pins the
shortcut against protocol.KZG.prove_point itself). Nothing here calls the code under test."""
import functools
import random

from pyoracle import protocol
from pyoracle.curves import BN254, BN254_R

SECRET = 100
R = BN254_R


@functools.lru_cache(maxsize=None)
def oracle(N):
    """protocol.KZG(N) without its N Lagrange points (N scalar multiplications that quotient() never
    reads): the object's other fields as protocol.KZG.__init__ sets them"""
    k = protocol.KZG.__new__(protocol.KZG)
    k.curve, k.secret, k.size = BN254, SECRET, N
    k.pre = protocol.PrecomputedLagrange(N, BN254)
    return k


@functools.lru_cache(maxsize=None)
def scalars(N):
    return tuple(protocol.kzg_lagrange_scalars(N, SECRET))


@functools.lru_cache(maxsize=None)
def omega(N):
    return protocol.group_gen(N)


@functools.lru_cache(maxsize=None)
def row(N, width, seed):
    """a random data row (a tuple: the cache keys on it)"""
    rng = random.Random(1000 * N + seed)
    return tuple(rng.randrange(R) for _ in range(width))


@functools.lru_cache(maxsize=None)
def quotient(N, evals, point):
    """(q, y) of protocol.KZG.quotient; raises IndexError / ZeroDivisionError / ValueError where
    the reference panics"""
    q, y = oracle(N).quotient(point, protocol.LagrangeBasis(list(evals), N))
    return tuple(q), y


@functools.lru_cache(maxsize=None)
def expected(N, evals, point):
    """{"proof", "y"} of the opening"""
    q, y = quotient(N, evals, point)
    s = sum(c * v for c, v in zip(scalars(N), q)) % R
    return {"proof": BN254.mul(BN254.g, s) if s else None, "y": y}


def standard_points(N, width, seed=0):
    """the issue's nine openings per N: 0, N - 1, one in [width, N), N + 1, N + 7, r - 1, three random"""
    rng = random.Random(77 * N + seed)
    mid = width if width < N else N - 1
    return [0, N - 1, mid, N + 1, N + 7, R - 1] + [rng.randrange(N + 8, R) for _ in range(3)]
