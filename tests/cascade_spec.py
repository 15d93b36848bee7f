"""The specification of the two-stage decode (include/ldpc_hip.h ldpc_cascade): a batch is decoded by a first decoder, the frames it does
not converge on -- in ascending frame order, at most `capacity` of them -- are decoded again FROM THE CHANNEL LLRs by a second one, and
take that result entirely.  The stage decoders are functions llr [F][N] -> (bits [F][N], iters [F], converged [F], ...), so the same lines
compose any two shipped specifications, or any two contexts' own decode_batch.  No GPU is needed here."""
import numpy as np


def select(converged, capacity):
    """-> idx: the frames with converged == 0, ascending, cut to the first `capacity`"""
    return np.flatnonzero(np.asarray(converged) == 0)[:int(capacity)]


def compose(stage1, stage2, llr, capacity):
    """-> bits [F][N] uint8, iters [F] int32, converged [F] uint8, stage [F] uint8 (1 or 2), stats [3] uint32 = (frames that failed
    stage 1, frames sent to stage 2, frames sent and still not converged).  stage2 is not called when no frame goes on"""
    llr = np.asarray(llr)
    b1, i1, c1 = stage1(llr)[:3]
    bits, iters, conv = np.array(b1, np.uint8), np.array(i1, np.int32), np.array(c1).astype(np.uint8)
    stage = np.ones(len(llr), np.uint8)
    failed = int((conv == 0).sum())
    idx = select(conv, capacity)
    still = 0
    if len(idx):
        b2, i2, c2 = stage2(llr[idx])[:3]
        bits[idx], iters[idx], conv[idx], stage[idx] = b2, i2, np.asarray(c2).astype(np.uint8), 2
        still = int((conv[idx] == 0).sum())
    return bits, iters, conv, stage, np.array([failed, len(idx), still], np.uint32)
