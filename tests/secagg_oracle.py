"""The oracle of the secure-aggregation tests: numpy and Python integers only, nothing imported from
the package. Its own Philox-4x32-10 (pinned by the known answer for counter 0, key 0), and the
encode, mask and open of csrc/kernels/secagg.hip written from their definition:

  encode : d = fl32(x - c) (no centre: x), p = fl32(cs * d), r = rint(double(p) * 2^f) ties to even,
           q = int(r) for |r| <= lim = (2^31 - 1) // n, +-lim beyond (counted), 0 for NaN (counted);
           a row with cs == 0 is not read (q = 0, nothing counted)
  mask   : m(a, b, e), a <= b: word e & 3 of philox(counter (Q_lo, Q_hi, (a << 16) | b, round),
           key (seed_lo ^ TAG, seed_hi)), Q = e >> 2;
           y = q + m(i, i) + sum_{j in U, j != i} s_ij m(min, max)  mod 2^32, s_ij = +1 for i < j else -1
  open   : T = sum y - sum_{i in S} m(i, i) - sum_{i in S, d in D} s_id m(min, max)  mod 2^32,
           delta = float32(int32(T)) * 2^-f
"""
import numpy as np

M32 = 0xFFFFFFFF
TAG = 0x9B05688C
KNOWN_ANSWER = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # counter 0, key 0


def philox(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint64 arrays holding 32-bit words; the key words are Python ints."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def pair_mask(P, a, b, seed, rnd):
    """m(a, b, e) for e in [0, P): uint64 holding 32-bit words."""
    assert 0 <= a <= b < 65536
    q = np.arange((P + 3) // 4, dtype=np.uint64)
    r = philox(q & np.uint64(M32), q >> np.uint64(32), np.full_like(q, (a << 16) | b), np.full_like(q, rnd & M32),
               (seed & M32) ^ TAG, (seed >> 32) & M32)
    return np.stack(r, 1).reshape(-1)[:P]


def signed_pair(P, i, j, seed, rnd):
    """s_ij m(min, max, .) as int64: +m for i < j, -m for i > j."""
    m = pair_mask(P, min(i, j), max(i, j), seed, rnd).astype(np.int64)
    return m if i < j else -m


def f32(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def encode(rows, center, cs, n, frac_bits):
    """-> (q [G, P] int64, sat [G] int64)."""
    rows, cs = f32(rows), f32(cs)
    G, P = rows.shape
    lim = (2 ** 31 - 1) // n
    q = np.zeros((G, P), dtype=np.int64)
    sat = np.zeros(G, dtype=np.int64)
    with np.errstate(all="ignore"):
        for g in range(G):
            if cs[g] == 0:
                continue
            d = rows[g] if center is None else (rows[g] - f32(center)).astype(np.float32)
            p = (cs[g] * d).astype(np.float32)
            r = np.rint(p.astype(np.float64) * float(2 ** frac_bits))
            nan = np.isnan(r)
            over = nan | (np.abs(r) > lim)
            r = np.where(nan, 0.0, np.clip(r, -lim, lim))
            q[g] = r.astype(np.int64)
            sat[g] = int(over.sum())
    return q, sat


def to_i32(t):
    """int64 holding any integer -> its residue mod 2^32 as int32."""
    return (t & M32).astype(np.uint32).view(np.int32)


def mask(rows, center, cs, slot_client, cohort, frac_bits, seed, rnd):
    """-> (words [G, P] int32, sat [G] int64, q [G, P] int64)."""
    q, sat = encode(rows, center, cs, len(cohort), frac_bits)
    G, P = q.shape
    words = np.zeros((G, P), dtype=np.int32)
    for g, i in enumerate(slot_client):
        y = q[g] + pair_mask(P, i, i, seed, rnd).astype(np.int64)
        for j in cohort:
            if j != i:
                y = y + signed_pair(P, i, j, seed, rnd)
        words[g] = to_i32(y)
    return words, sat, q


def bare_masks(P, i, cohort, seed, rnd):
    """What client i uploads for q = 0."""
    y = pair_mask(P, i, i, seed, rnd).astype(np.int64)
    for j in cohort:
        if j != i:
            y = y + signed_pair(P, i, j, seed, rnd)
    return to_i32(y)


def dequant(T_i32, frac_bits):
    """float32(int32) rounds to nearest even; the power of two is exact."""
    return (np.asarray(T_i32, dtype=np.int32).astype(np.float32) * np.float32(2.0 ** -frac_bits)).astype(np.float32)


def open_(words, survivors, dropped, frac_bits, seed, rnd):
    """words [R, P] int32 -> delta [P] float32."""
    words = np.asarray(words, dtype=np.int32)
    P = words.shape[1]
    T = words.astype(np.int64).sum(0)
    for i in survivors:
        T = T - pair_mask(P, i, i, seed, rnd).astype(np.int64)
        for d in dropped:
            T = T - signed_pair(P, i, d, seed, rnd)
    return dequant(to_i32(T), frac_bits)


def plain_sum(q, frac_bits):
    """(float)(sum_g q_g) * 2^-f from the fixed-point updates alone: no Philox."""
    return dequant(to_i32(np.asarray(q, dtype=np.int64).sum(0)), frac_bits)
