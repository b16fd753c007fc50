"""The window of FusedAdamW.accumulate_steps (csrc/kan_accum.hip: k_grad_accumulate, k_accum_gate) in numpy float32, and the layouts the tests run it
on.  Restated from include/kanconv.h, not from the kernel: micro-step 0 COPIES the gradient, every later one adds to the accumulator in call
order (one fp32 add per element), the last one multiplies the sum by np.float32(1.0 / k).  A segment without a gradient is zero-filled at
micro-step 0, left alone in the middle and, at the last micro-step, only scaled.  tests/test_accum.py and tests/test_gpu_accum.py import this."""
import numpy as np

ALIGN, CHUNK = 64, 8192                                # optim.py: _ALIGN, _CHUNK

# (elements, kind).  Sizes at the float4 tail (1, 3, 4, 5), around the 8192-element chunk (8191, 8192, 8193) and over three chunks with a tail
# (2 * 8192 + 7); "null": the segment never has a gradient address; "view": the gradient is buf[1:1 + n] -- 4-byte but not 16-byte aligned, the
# scalar path of the kernel.
KERNEL_LAYOUT = [(1, "own"), (3, "own"), (4, "own"), (5, "view"), (7, "null"), (8191, "own"), (8192, "own"), (8193, "view"), (2 * 8192 + 7, "own")]
SENTINEL_BITS = 0x7FC00ABC                             # a quiet NaN with a payload: what the accumulator and the padding hold before the first window


def flat_layout(sizes):
    """seg_off (64-element alignment), seg_n, chunk_seg, chunk_start and the row length, as FusedAdamW._flatten lays a group out."""
    seg_off, n = [], 0
    for size in sizes:
        seg_off.append(n)
        n += (size + ALIGN - 1) // ALIGN * ALIGN
    chunk_seg = [i for i, size in enumerate(sizes) for _ in range(0, size, CHUNK)]
    chunk_start = [s0 for size in sizes for s0 in range(0, size, CHUNK)]
    return dict(seg_off=seg_off, seg_n=list(sizes), chunk_seg=chunk_seg, chunk_start=chunk_start, n=n)


def padding_mask(layout):
    """True at the elements of the row that belong to no segment."""
    mask = np.ones(layout["n"], dtype=bool)
    for off, size in zip(layout["seg_off"], layout["seg_n"]):
        mask[off:off + size] = False
    return mask


def micro_step(acc, g, m, k):
    """One segment, one micro-step: the new accumulator (float32 array) from the old one (`acc`; never read at m == 0) and the gradient `g`
    (float32 array, or None: no gradient address in this call)."""
    assert 0 <= m < k
    s = np.float32(1.0 / k)
    if m == 0:
        return np.zeros_like(acc) if g is None else g.astype(np.float32, copy=True)
    if m < k - 1:
        return acc if g is None else acc + g
    return acc * s if g is None else (acc + g) * s


def window_mean(grads):
    """The accumulator after a whole window of len(grads) micro-steps of one parameter; None if no micro-step had a gradient."""
    k = len(grads)
    if all(g is None for g in grads):
        return None
    acc = np.zeros_like(next(g for g in grads if g is not None), dtype=np.float32)
    for m, g in enumerate(grads):
        acc = micro_step(acc, None if g is None else np.asarray(g, dtype=np.float32), m, k)
    return acc


def gate_model(micro, k, seen, addr):
    """(gated table, seen afterwards, counter afterwards) of one group for one kan_accum_gate call."""
    if micro + 1 == k:
        return [a if s else 0 for a, s in zip(addr, seen)], [0] * len(seen), 0
    return [0] * len(seen), list(seen), micro + 1
