"""Test helper: BLS12-381 G2 in Python integers (the M-type twist y^2 = x^3 + 4 (1 + u) over
Fq2 = Fq[u]/(u^2 + 1)). Only what the KZG-verification fixtures and tests need: the generator H,
k * Q, and a point of the twist outside the order-r subgroup. Points are ((x0, x1), (y0, y1))
with x = x0 + x1 u, the identity is None -- the layout of vkzg.scheme's G2 arguments."""
from pyoracle.curves import BLS_P as P, BLS_R as R, sqrt_mod

H = ((int("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8", 16),
      int("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e", 16)),
     (int("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801", 16),
      int("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be", 16)))


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


B2 = f2mul((4, 0), (1, 1))


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
    """a point of the twist whose order does not divide r (the twist has a large cofactor)."""
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
