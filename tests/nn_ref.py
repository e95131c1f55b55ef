"""The nearest-training-image check (relativisticgan_amd/neighbours.py, csrc/nn.hip) restated in
numpy int64, the plain way: the whole Q x R matrix of squared distances is formed.  Everything is
exact, so the tests compare integers with == and the float64 results with == too (the same
integers through the same float64 formulas)."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
MAX_ROW_BYTES = 12288
SIDES = (8, 16, 32, 64)


def row_bytes(C, s):
    return (C * s * s + 63) // 64 * 64


def pack(u8, s):
    """uint8 [N][C][S][S] -> (desc int8 [N][row_bytes], norm int64 [N]): the rounded f x f box mean
    (halves up) minus 128 in (c, y, x) order, zero pad."""
    u8 = np.asarray(u8)
    N, C, S, _ = u8.shape
    assert u8.dtype == np.uint8 and s in SIDES and S % s == 0 and S // s <= 32
    f = S // s
    box = u8.astype(np.int64).reshape(N, C, s, f, s, f).sum(axis=(3, 5))
    v = (box + (f * f) // 2) // (f * f) - 128
    desc = np.zeros((N, row_bytes(C, s)), dtype=np.int8)
    desc[:, :C * s * s] = v.reshape(N, -1)
    return desc, (desc.astype(np.int64) ** 2).sum(axis=1)


def dist2(a, b):
    """int64 [Q][R]: the squared distances of the rows of a to the rows of b."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    return na[:, None] + nb[None, :] - 2 * (a @ b.T)


def excluded(Q, R, self_offset):
    """bool [Q][R]: r == q + self_offset (None: nothing is)."""
    if self_offset is None:
        return np.zeros((Q, R), dtype=bool)
    return np.arange(R)[None, :] == np.arange(Q)[:, None] + self_offset


def topk(a, b, k, self_offset=None):
    """(dist, idx) int64 [Q][k]: the k smallest keys (d2 << 32) | r of the rows not excluded,
    ascending; the tail beyond the rows that remain is (INT32_MAX, -1)."""
    return topk_d(dist2(a, b), k, self_offset)


def topk_d(d, k, self_offset=None):
    """``topk`` of a given matrix of squared distances."""
    d = np.asarray(d, dtype=np.int64)
    Q, R = d.shape
    key = (d << 32) | np.arange(R, dtype=np.int64)[None, :]
    none = np.int64(2 ** 63 - 1)
    key = np.where(excluded(Q, R, self_offset), none, key)
    key = np.sort(key, axis=1)[:, :k]
    if key.shape[1] < k:
        key = np.concatenate([key, np.full((Q, k - key.shape[1]), none)], axis=1)
    missing = key == none
    return np.where(missing, INT32_MAX, key >> 32), np.where(missing, -1, key & 0xFFFFFFFF)


def covered(a, b, radius, self_offset=None):
    """int64 [Q]: 1 where some row r of b that is not excluded has d2(q, r) <= radius[r]."""
    return covered_d(dist2(a, b), radius, self_offset)


def covered_d(d, radius, self_offset=None):
    """``covered`` of a given matrix of squared distances."""
    d = np.asarray(d, dtype=np.int64)
    hit = (d <= np.asarray(radius, dtype=np.int64)[None, :]) & ~excluded(*d.shape, self_offset)
    return hit.any(axis=1).astype(np.int64)


def median(x):
    v = np.sort(np.asarray(x, dtype=np.float64))
    n = v.size
    return float(v[n // 2]) if n % 2 else (float(v[n // 2 - 1]) + float(v[n // 2])) / 2.0


def report(real_u8, fake_u8, s, k):
    """The five numbers for N reals and N fakes (uint8 [N][C][S][S] each), and cross's (dist, idx)."""
    real_u8, fake_u8 = np.asarray(real_u8), np.asarray(fake_u8)
    N, C = real_u8.shape[:2]
    assert fake_u8.shape == real_u8.shape and N >= k + 1
    D = C * s * s
    r, _ = pack(real_u8, s)
    f, _ = pack(fake_u8, s)
    real_knn, fake_knn, cross = topk(r, r, k, 0), topk(f, f, k, 0), topk(f, r, k)
    out = {"fake_nn": median(np.sqrt(cross[0][:, 0].astype(np.float64) / D)),
           "real_nn": median(np.sqrt(real_knn[0][:, 0].astype(np.float64) / D))}
    out["ratio"] = out["fake_nn"] / out["real_nn"] if out["real_nn"] > 0 else float("inf")
    out["precision"] = float(covered(f, r, real_knn[0][:, k - 1]).sum()) / N
    out["recall"] = float(covered(r, f, fake_knn[0][:, k - 1]).sum()) / N
    return out, cross


def grid(real_u8, fake_u8, idx, k):
    """uint8 [(S + 2) 8 + 2][(S + 2)(k + 1) + 2][C]: row i = fake i, then reals idx[i][0..k-1]."""
    real_u8, fake_u8 = np.asarray(real_u8), np.asarray(fake_u8)
    C, S = fake_u8.shape[1:3]
    out = np.zeros(((S + 2) * 8 + 2, (S + 2) * (k + 1) + 2, C), dtype=np.uint8)
    for i in range(min(8, fake_u8.shape[0])):
        cells = [fake_u8[i]] + [real_u8[int(r)] if r >= 0 else None for r in idx[i][:k]]
        for j, cell in enumerate(cells):
            if cell is not None:
                y, x = 2 + i * (S + 2), 2 + j * (S + 2)
                out[y:y + S, x:x + S] = cell.transpose(1, 2, 0)
    return out


def to_u8(x):
    """Floats in [-1, 1] as the PNG writer quantises x * .5 + .5 (images.to_u8: fp32 arithmetic,
    times 255 plus .5, clamped, truncated)."""
    x = np.asarray(x, dtype=np.float32)
    v = (x * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0) + np.float32(0.5)
    return np.clip(v, 0, 255).astype(np.uint8)
