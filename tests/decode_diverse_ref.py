"""Numpy restatement of the group-diverse form of dec_sent_kernel (csrc/decode.hip, `diverse_groups` of include/s2t_hip.h).

`diverse_candidates` forms the 2 beam ranked candidates of one sentence from the rows' candidate lists the way the kernel does -- the
groups in order, every group on the list entries of its own rows, each entry's value lowered by strength x (how many candidates the
earlier groups of this step took with that token), in float32 as a rounded product and a rounded subtraction -- and `sent_step_diverse`
feeds them to the unchanged bookkeeping of decode_ref.sent_step (see there how), so that nothing of the bookkeeping is restated here.

What it restates of the reference (fairseq/search.py:103-161): group g holds the slots g, g + G, ...; at step 0 it holds slot g alone
(every slot is the same there; the lists come from the sentence's first row, the only one the row launch fills at step 0); a group takes
its 2 beam / G best (value descending, then (row's index within the group) V + column ascending); the counts cover all 2 beam / G
candidates of every earlier group (diversity_buf.scatter_add_); candidate j of group g is overall candidate j G + g (stack(dim=2).view).
That the rows' 2 beam best are enough for any strength >= 0 is pinned by tests/test_decode_diverse_cpu.py against the reference's outputs.

`count_all`, `interleave`, `sign`: the three deliberately wrong variants of the CPU test (count only the first beam / G candidates of a
group; concatenate the groups' candidates; add the penalty).
"""
import numpy as np

import decode_ref as R


def diverse_candidates(cand_val, cand_idx, beam, V, G, strength, first, count_all=True, interleave=True, sign=-1.0):
    """cand_val float32 [beam, 2 beam] / cand_idx int [beam, 2 beam]: one sentence's row lists (value descending, column ascending).
    first: step 0 without step0_all_slots.  Returns (val float32 [2 beam], tok [2 beam], slot [2 beam]) in rank order."""
    K2, mg = 2 * beam, beam // G
    kg = min(2 * mg, (V if first else mg * V) - 1)
    lam = np.float32(strength)
    val = np.full(G * kg, -np.inf, np.float32)
    tok = np.zeros(G * kg, np.int64)
    slot = np.zeros(G * kg, np.int64)
    taken = []                                                   # tokens of the candidates the earlier groups took
    for g in range(G):
        rows = [0] if first else [g + i * G for i in range(mg)]
        ent = []
        for i, r in enumerate(rows):
            for e in range(K2):
                v, c = np.float32(cand_val[r, e]), int(cand_idx[r, e])
                cnt = np.float32(sum(1 for x in taken if x == c))
                with np.errstate(invalid="ignore"):
                    pen = np.float32(lam * cnt)                  # rounded product ...
                    pv = np.float32(v - pen) if sign < 0 else np.float32(v + pen)      # ... then a rounded subtraction
                ent.append((pv, i * V + c, g if first else r, c))
        ent.sort(key=lambda x: (-x[0], x[1]))
        ent = ent[:kg]
        for j, (pv, _, r, c) in enumerate(ent):
            rank = j * G + g if interleave else g * kg + j
            val[rank], tok[rank], slot[rank] = pv, c, r
        taken += [x[3] for x in (ent if count_all else ent[:mg])]
    return val, tok, slot


def sent_step_diverse(st, cand_val, cand_idx, beam, V, eos, max_len, G, strength):
    """One launch of the diverse dec_sent_kernel on host state `st` (decode_ref.new_state's arrays, modified in place); cand_val [N, 2 beam]
    float32 / cand_idx: every row's list.  G <= 1: decode_ref.sent_step itself.

    decode_ref.sent_step merges the lists it is given by (value descending, flat index ascending) and does the bookkeeping on the
    result.  The ranked candidates are not in value order (the groups are interleaved), so they are handed over in the first row's
    list with strictly decreasing stand-in values 2 beam - rank and the index slot V + token, which decode_ref decodes to (parent
    slot, token); the other rows hold -inf entries that are never taken.  The stand-ins are then replaced, in the records the step
    wrote, by the candidates' own values.  A -inf candidate is never an EOS hypothesis (decode_ref tests the value): it is handed
    over with a token that is not EOS and gets its own token back the same way."""
    if G <= 1:
        return R.sent_step(st, cand_val, cand_idx, beam, V, eos, max_len, False)
    B, K2 = st["steps"].shape[0], 2 * beam
    N = B * beam
    cv = np.full((N, K2), -np.inf, np.float32)
    ci = np.zeros((N, K2), np.int64)
    ranked, before = {}, {}
    not_eos = (eos + 1) % V
    for s in range(B):
        n0, t = s * beam, int(st["steps"][s])
        if t > max_len:
            continue
        val, tok, slot = diverse_candidates(cand_val[n0:n0 + beam], cand_idx[n0:n0 + beam], beam, V, G, strength, t == 0)
        assert val.shape[0] == K2, "V >= 2 beam + 1 (the limits of include/s2t_hip.h): every group takes 2 beam / G"
        ranked[s], before[s] = (val, tok, slot, t), int(st["nfin"][s])
        cv[n0] = (K2 - np.arange(K2)).astype(np.float32)
        ci[n0] = slot * V + np.where(np.isneginf(val), not_eos, tok)
    # step0_all = True: decode_ref then reads every row's list at step 0 too; the lists of the other rows are empty (-inf) here
    R.sent_step(st, cv, ci, beam, V, eos, max_len, True)
    for s, (val, tok, slot, t) in ranked.items():
        n0 = s * beam
        for place in range(beam):
            rank = K2 - int(st["cum_hist"][t + 1, n0 + place])
            assert int(st["par_hist"][t + 1, n0 + place]) == n0 + int(slot[rank])
            st["cum_hist"][t + 1, n0 + place] = val[rank]
            st["tok_hist"][t + 1, n0 + place] = tok[rank]
        for f in range(before[s], int(st["nfin"][s])):
            st["fin_score"][s, f] = val[K2 - int(st["fin_score"][s, f])]
