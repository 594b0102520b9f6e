"""The bank mix (bfir_engine_set_coeff_matrix_bank_mix and its kin; k_bank_mix in csrc/bankmix.hip) restated in NumPy.

IEEE single and double multiply and add are what NumPy does on float32 / float64 arrays, one rounding per operation, so the
restatement is exact to the bit as long as no product or sum is subnormal (the one place where a device may differ by mode);
mix_row asserts that its result holds none."""
import numpy as np


def converted(w, dtype):
    """A weight as the call converts it: once, to the working precision."""
    with np.errstate(over="ignore", under="ignore"):
        return np.dtype(dtype).type(w)


def mix_row(rows, counts, weights, dtype, B):
    """The row a mix writes and its partition count.

    rows[j]: the B partitions of term j's entry as bank_read returns them ([B][2 L], zeros at and past its count), or None for
    an entry of -1; counts[j]: that entry's partition count (0: empty; ignored for None); weights[j]: the weight as given to
    the call.  A term is live iff it has an entry and its converted weight is not zero.  Partition p of the result is
    fl(w h) of the first live term with count > p, then fl(. + fl(w h)) of the later ones in listed order; the count is the
    largest among the live terms, and partitions at and past it are zeros."""
    dtype = np.dtype(dtype)
    ws = [converted(w, dtype) for w in weights]
    live = [j for j in range(len(ws)) if rows[j] is not None and ws[j] != 0]
    assert all(counts[j] >= 1 for j in live), "a live term names an empty entry: the call refuses it"
    c = max([counts[j] for j in live], default=0)
    n = next((np.asarray(r).shape[1] for r in rows if r is not None), 0)
    out = np.zeros((B, n), dtype)
    for p in range(c):
        acc = None
        for j in live:
            if counts[j] <= p:
                continue
            h = np.asarray(rows[j][p])
            assert h.dtype == dtype
            prod = ws[j] * h
            assert prod.dtype == dtype
            acc = prod if acc is None else acc + prod      # the first product starts the sum: no 0 + ...
            assert acc.dtype == dtype and not _subnormal(prod) and not _subnormal(acc), \
                "a subnormal product or sum: the restatement would depend on the denormal mode"
        out[p] = acc
    return out, c


def _subnormal(a):
    return bool(np.any((a != 0) & (np.abs(a) < np.finfo(a.dtype).tiny)))
