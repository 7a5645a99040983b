"""numpy definitions of the order-fixed backward (include/prcnn_hip.h: prcnn_scatter_plan and the two *_grad_ordered entries).
A helper, not a test: tests/test_scatter_ref.py pins it against a literal per-slot loop, tests/test_gpu_ordered_backward.py pins the
kernels against it."""
import numpy as np


def plan(idx, n):
    """idx (b, slots) integers -> offsets (b, n+1) i32, entries (b, slots) i32: per cloud the stable argsort of the in-range slots
    and the cumulative bincount; entries behind offsets[i][n] are -1 here (unspecified in the library)."""
    idx = np.asarray(idx)
    idx = idx.reshape(idx.shape[0], int(np.prod(idx.shape[1:]))).astype(np.int64)      # (b = 0 keeps its slot count)
    b, slots = idx.shape
    offsets = np.zeros((b, n + 1), np.int32)
    entries = np.full((b, slots), -1, np.int32)
    for i in range(b):
        inside = np.nonzero((idx[i] >= 0) & (idx[i] < n))[0]
        order = inside[np.argsort(idx[i][inside], kind="stable")]
        entries[i, :len(order)] = order
        offsets[i, 1:] = np.cumsum(np.bincount(idx[i][inside], minlength=n)[:n])
    return offsets, entries


def ordered_sum(offsets, entries, terms, n, chunk):
    """terms (b, c, slots) f32 -> (b, c, n) f32.  A list is cut into chunks of `chunk` entries; each chunk is summed left to right
    from +0.0f, the chunk sums are added left to right from +0.0f.  Vectorised over destinations by rank within the list: round r
    adds every list's r-th term (f32 adds, one rounding each)."""
    terms = np.asarray(terms, np.float32)
    b, c, _ = terms.shape
    out = np.zeros((b, c, n), np.float32)
    for i in range(b):
        off = offsets[i].astype(np.int64)
        lens = off[1:] - off[:-1]
        tot, acc = np.zeros((c, n), np.float32), np.zeros((c, n), np.float32)
        for r in range(int(lens.max()) if n else 0):
            live = np.nonzero(lens > r)[0]
            acc[:, live] = acc[:, live] + terms[i][:, entries[i][off[live] + r]]
            if (r + 1) % chunk == 0:                                 # these lists close a chunk
                tot[:, live] = tot[:, live] + acc[:, live]
                acc[:, live] = 0.0
        open_chunk = np.nonzero(lens % chunk != 0)[0]
        tot[:, open_chunk] = tot[:, open_chunk] + acc[:, open_chunk]
        out[i] = tot
    return out


def interp_terms(grad_out, weight):
    """grad_out (b, c, n) f32, weight (b, n, 3) f32 -> terms (b, c, 3n) f32: slot s is unknown point s // 3, the f32 product"""
    grad_out, weight = np.asarray(grad_out, np.float32), np.asarray(weight, np.float32)
    b, c, n = grad_out.shape
    return (np.repeat(grad_out, 3, axis=2) * weight.reshape(b, 1, 3 * n)).astype(np.float32)


def literal(idx, terms, n, chunk):
    """The definition as a per-slot Python loop (slow: small shapes only) -> (offsets, lists, sums)"""
    idx = np.asarray(idx).reshape(len(idx), -1)
    terms = np.asarray(terms, np.float32)
    b, slots = idx.shape
    c = terms.shape[1]
    offsets = np.zeros((b, n + 1), np.int32)
    lists = [[[] for _ in range(n)] for _ in range(b)]
    sums = np.zeros((b, c, n), np.float32)
    for i in range(b):
        for s in range(slots):
            k = int(idx[i][s])
            if 0 <= k < n:
                lists[i][k].append(s)
        for k in range(n):
            offsets[i][k + 1] = offsets[i][k] + len(lists[i][k])
            for ch in range(c):
                total = np.float32(0.0)
                for at in range(0, len(lists[i][k]), chunk):
                    part = np.float32(0.0)
                    for s in lists[i][k][at:at + chunk]:
                        part = np.float32(part + terms[i][ch][s])
                    total = np.float32(total + part)
                sums[i][ch][k] = total
    return offsets, lists, sums


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)
