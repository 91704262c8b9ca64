"""Test helper: BN254 G2 in Python integers (the D-type twist y^2 = x^3 + 3 / (9 + u) over
Fq2 = Fq[u]/(u^2 + 1)). Only what the KZG-verification fixtures and tests need: the generator H,
k * Q, and a point of the twist outside the order-r subgroup. Points are ((x0, x1), (y0, y1))
with x = x0 + x1 u, the identity is None -- the layout of vkzg.scheme's G2 arguments."""
from pyoracle.curves import BN254_P as P, BN254_R as R, sqrt_mod

H = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
      11559732032986387107991004021392285783925812861821192530917403151452391805634),
     (8495653923123431417604973247489272438418190587263600148770280649306958101930,
      4082367875863433681332203403145435568316851327593401208105741076214120093531))


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2sqrt(a):
    """a square root in Fq2 or None (p = 3 mod 4: the complex method)."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = sqrt_mod(a0, P)
        if s is not None:
            return (s, 0)
        return (0, sqrt_mod(-a0 % P, P))
    alpha = sqrt_mod((a0 * a0 + a1 * a1) % P, P)
    if alpha is None:
        return None
    half = pow(2, -1, P)
    for delta in ((a0 + alpha) * half % P, (a0 - alpha) * half % P):
        x0 = sqrt_mod(delta, P)
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, P) % P)
            if f2mul(r, r) == (a0, a1):
                return r
    return None


B2 = f2mul((3, 0), f2inv((9, 1)))


def on_twist(Q):
    if Q is None:
        return True
    x, y = Q
    return f2mul(y, y) == f2add(f2mul(f2mul(x, x), x), B2)


def neg(Q):
    return None if Q is None else (Q[0], ((-Q[1][0]) % P, (-Q[1][1]) % P))


def add(A, Bq):
    if A is None:
        return Bq
    if Bq is None:
        return A
    (x1, y1), (x2, y2) = A, Bq
    if x1 == x2:
        if y1 != y2 or y1 == (0, 0):
            return None
        lam = f2mul(f2mul((3, 0), f2mul(x1, x1)), f2inv(f2add(y1, y1)))
    else:
        lam = f2mul(f2sub(y2, y1), f2inv(f2sub(x2, x1)))
    x3 = f2sub(f2sub(f2mul(lam, lam), x1), x2)
    return (x3, f2sub(f2mul(lam, f2sub(x1, x3)), y1))


def mul(Q, k):
    """k * Q for any integer k >= 0 (no reduction mod r: Q may lie outside the subgroup)."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, Q)
    return acc


def outside_subgroup():
    """a point of the twist whose order does not divide r (the twist's cofactor is 2p - r)."""
    x0 = 1
    while True:
        x = (x0, 1)
        y = f2sqrt(f2add(f2mul(f2mul(x, x), x), B2))
        if y is not None:
            Q = (x, y)
            assert on_twist(Q)
            if mul(Q, R) is not None:
                return Q
        x0 += 1
