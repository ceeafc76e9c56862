"""numpy restatement of llmk_score's outputs (include/llmk.h) from the logits of every position, in float64:
logprob[i] = z[target_i - 1] - lse(z), 0.0 where target_i == 0; argmax[i] = the 1-based FIRST maximum of z."""
import numpy as np


def lse(logits):
    """log-sum-exp of every row, float64; -inf for a row with no entry above -inf"""
    z = np.asarray(logits, np.float64)
    z = z.reshape(-1, z.shape[-1])
    m = z.max(axis=1)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.exp(z - ms[:, None]).sum(axis=1)), m)


def default_targets(tokens):
    """the tokens shifted by one, and 0 (no target) for the last position"""
    t = np.asarray(tokens, np.int32)
    return np.append(t[1:], 0).astype(np.int32)


def score(logits, targets):
    """(logprob [n] float64, argmax [n] int32, 1-based) of logits [n][V] and 1-based targets [n] (0 = none)"""
    z = np.asarray(logits, np.float64)
    z = z.reshape(-1, z.shape[-1])
    tg = np.asarray(targets, np.int64)
    assert tg.shape == (len(z),) and (tg >= 0).all() and (tg <= z.shape[1]).all()
    picked = z[np.arange(len(z)), np.maximum(tg, 1) - 1]
    lp = np.where(tg > 0, picked - lse(z), 0.0)
    return lp, (np.argmax(z, axis=1) + 1).astype(np.int32)      # (np.argmax returns the first maximum)
