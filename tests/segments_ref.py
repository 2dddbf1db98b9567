"""Float64 numpy reference of the rollout-segment kernels (csrc/cm_segments.hip): the targets of a [P,T] batch of segments with
episode ends inside and a bootstrapped end, the batch-wide advantage normalisation and the episode bookkeeping across segments.
Plain loops, no GPU; tests/test_segments_cpu.py holds it to the textbook formulas piece by piece.

Conventions: rewards / dones / baselines are [P,T]; dones[p,t] set means the episode ended WITH step t (nothing behind it counts
for step t or any step before it); v_last[p] is the critic's value of the state behind the row's last step.  The recurrences take
their coefficients as arguments - gamma_adv (the delta's discount), gl (the accumulator's gamma * lambda) and gamma_ret (the
return's discount) - because the kernel is specified with cm_gae's and cm_discount_returns' arithmetic: the delta and gl are
built from gamma and lambda rounded to f32 (gl is their f32 product), the return recurrence uses the f64 gamma."""
import numpy as np

U = 2.0 ** -24                                              # unit roundoff of f32


def kernel_coefficients(gamma, lam):
    """(gamma_adv, gl, gamma_ret) as cm_segment_targets uses them for the doubles gamma, lam it is given."""
    g32, l32 = np.float32(gamma), np.float32(lam)
    return float(g32), float(np.float32(g32 * l32)), float(gamma)


def pieces(done_row):
    """[(first, last)] of the pieces a row falls into: each ends with a done, the last one with the row."""
    out, first = [], 0
    T = len(done_row)
    for t in range(T):
        if done_row[t] or t == T - 1:
            out.append((first, t))
            first = t + 1
    return out


def segment_targets(rewards, dones, baselines, v_last, gamma_adv, gl, gamma_ret):
    """-> (adv, returns, adv_terms), all [P,T] float64.  adv_terms[p,t] = sum over the rest of t's piece of
    gl^(k-t) * (|r_k| + gamma_adv * |V_{k+1}| + |V_k|): the size of what the f32 deltas are made of (the tests' bound)."""
    r, v = np.asarray(rewards, np.float64), np.asarray(baselines, np.float64)
    d, vl = np.asarray(dones).astype(bool), np.asarray(v_last, np.float64)
    P, T = r.shape
    adv, ret, terms = np.zeros((P, T)), np.zeros((P, T)), np.zeros((P, T))
    for p in range(P):
        acc, y, vnext, tt = 0.0, vl[p], vl[p], 0.0
        for t in range(T - 1, -1, -1):
            if d[p, t]:
                acc, y, vnext, tt = 0.0, 0.0, 0.0, 0.0
            delta = r[p, t] + gamma_adv * vnext - v[p, t]
            acc = delta + gl * acc
            tt = (abs(r[p, t]) + gamma_adv * abs(vnext) + abs(v[p, t])) + gl * tt
            y = r[p, t] + gamma_ret * y
            adv[p, t], ret[p, t], terms[p, t] = acc, y, tt
            vnext = v[p, t]
    return adv, ret, terms


def adv_bound(adv, terms):
    """The derived tolerance of the f32 advantages: the final cast (U |A_t|) + every f32 delta of the piece's rest - the cast of
    r, the product gamma * V, the sum and the difference: at most 4 U times the size of its terms."""
    return U * np.abs(adv) + 4 * U * terms


def textbook_gae(r, v, v_end, gamma, lam):
    """GAE(gamma, lambda) of ONE episode piece by its definition, A_t = sum_l (gamma lam)^l delta_{t+l} with
    delta_k = r_k + gamma V_{k+1} - V_k and V behind the last step = v_end (0 for a terminal state)."""
    n = len(r)
    vv = np.append(np.asarray(v, np.float64), v_end)
    delta = np.asarray(r, np.float64) + gamma * vv[1:] - vv[:-1]
    return np.array([sum((gamma * lam) ** l * delta[t + l] for l in range(n - t)) for t in range(n)])


def textbook_returns(r, v_end, gamma):
    """R_t = sum_l gamma^l r_{t+l} + gamma^(n-t) v_end of ONE episode piece."""
    n = len(r)
    return np.array([sum(gamma ** l * r[t + l] for l in range(n - t)) + gamma ** (n - t) * v_end for t in range(n)])


def adv_normalize(x, eps):
    """(x - mean) / sqrt(var + eps) over ALL values, biased variance, float64."""
    x = np.asarray(x, np.float64)
    m = x.mean()
    return (x - m) / np.sqrt(((x - m) ** 2).mean() + eps)


def draw_dones(P, T, rng, p=0.1):
    """dones [P,T] drawn with probability p, then overridden so that - as far as P and T allow - row 0 has no done, row 1 its
    only done at the last step, row 2 a done at step 0 and row 3 two dones in a row."""
    d = rng.random((P, T)) < p
    d[0] = False
    if P > 1:
        d[1] = False
        d[1, T - 1] = True
    if P > 2:
        d[2, 0] = True
        if P == 3 and T > 1:                                # the small case: the pair of dones goes here as well
            d[2, 1] = True
    if P > 3 and T > 2:
        d[3, 1:3] = True
    return d


def episodes(reward, done, details, success, gamma, carry=None):
    """The episodes that end within reward / done [T,B], details [T,B,6], success [T,B], per env from `carry` on (None: fresh
    envs) -> (list of per-episode dicts in (env, end step) order, the carry behind the last slot)."""
    T, B = reward.shape
    out = []
    carry = [dict(ret=0.0, disc=0.0, gp=1.0, n=0, det=np.zeros(5, np.int64)) for _ in range(B)] if carry is None else carry
    for b in range(B):
        c = carry[b]
        for t in range(T):
            c["ret"] += reward[t, b]
            c["disc"] += c["gp"] * reward[t, b]
            c["gp"] *= gamma
            c["n"] += 1
            c["det"] = c["det"] + details[t, b, :5].astype(np.int64)
            if done[t, b]:
                out.append(dict(ret=c["ret"], disc=c["disc"], n=c["n"], det=c["det"], success=int(success[t, b]), env=b, end=t))
                carry[b] = c = dict(ret=0.0, disc=0.0, gp=1.0, n=0, det=np.zeros(5, np.int64))
    return out, carry


def episode_table(eps):
    """cm_segment_episodes' row (the columns of _lib.SEG_COLUMNS) of a list of episodes()."""
    ret = np.array([e["ret"] for e in eps], np.float64)
    row = dict(count=float(len(eps)), ret_sum=float(ret.sum()), ret_sumsq=float((ret ** 2).sum()),
               ret_min=float(ret.min()) if len(eps) else np.inf, ret_max=float(ret.max()) if len(eps) else -np.inf,
               disc_sum=float(sum(e["disc"] for e in eps)), len_sum=float(sum(e["n"] for e in eps)),
               success=float(sum(e["success"] for e in eps)))
    for k in range(5):
        row[f"details_{k}"] = float(sum(int(e["det"][k]) for e in eps))
    return row
