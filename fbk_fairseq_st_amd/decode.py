"""Device-resident beam search over one incremental decoder, or over an ensemble of up to eight.

The search loop of the reference (fairseq/sequence_generator.py:243-447 with fairseq/search.py:55-83 and the incremental
TransformerDecoder, fairseq/models/transformer.py:674-782) as `3 * layers + 4` kernel launches per decoding step, all of them
inside libs2t_hip.so (csrc/decode.hip, include/s2t_hip.h `s2t_decode_*`): the host launches one recorded step after the other
and looks at the `finished` flags every few steps.  Nothing of the state is re-ordered when the beam changes: the kernels follow
an ancestor table, the encoder-side K/V exist once per sentence, and the hypotheses are read back at the end by walking the
recorded (token, parent, cumulative score) triples.

An ensemble (`EnsembleDecodeSession`, `s2t_decode_*_ensemble`) shares ONE search state: every member runs its own launches up to its
logits into its own buffers, one member after the other, then one row launch takes the log of the members' mean probability before the
score rules and one sentence launch does the bookkeeping and embeds the chosen tokens for every member:
`sum_j (3 * layers_j + 2) + 2` launches per step.  The members may differ in width, depth and encoder length.

`SequenceGenerator` (sequence_generator.py) takes this path for one model or an ensemble with the plain, the hierarchical or the
group-diverse beam search (`diverse_groups`: the per-sentence launch forms the groups' penalised candidates from the same row lists), with n-gram blocking (n >= 2) and prefix tokens (without EOS) as two more score rules of the per-row launch
(`s2t_decode_step_rules`), or with the sampling search (`sampling`: each row draws its one candidate inside the per-row launch,
`s2t_decode_step_sample`).  Two options ride in `S2TDecodeExtras` behind the `s2t_decode_*_ex` calls: `--layernorm-embedding` members
(the rows of every decoder input are normalised where they are written) and, for one model, `retain_attention`: the last layer's
encoder-attention launch also stores its per-head probabilities, the final LayerNorm launch averages them into one record per step,
and `hypotheses` gathers every hypothesis' `[Ts, len]` attention from those records along its parent links.  The generator keeps its
step-by-step path (the same decoder kernels + torch index bookkeeping) for an ensemble that returns attention, a prefix that holds
EOS, n-gram size 1, members of different dtypes and any member outside the shape limits.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import lib as L

ATTN_HIST_CAP = 1 << 30              # bytes of attention records ((max_len + 1) * N * Ts * 4) a session accepts: beyond, `ok` is False
POLL_STEPS = 8                       # the host reads the `finished` flags every POLL_STEPS steps (one small D2H copy + sync)
LDS_CAP = 152 * 1024                 # csrc/decode.hip LDS_CAP


def _pick_hidden_slice(ffn, B):
    """hidden units per F-launch workgroup (64, 128 or 256): enough (sentence, slice) workgroups for the 256 CUs"""
    forced = int(os.environ.get("S2T_DECODE_HS", "0"))              # diagnostic: tools/decode_stamps.py compares the slice widths
    if forced and ffn % forced == 0:
        return forced
    for hs in ((128, 64, 256) if B * (ffn // 128) >= 128 else (64, 128, 256)):
        if ffn % hs == 0:
            return hs
    return 0


class _Member:
    """One model's share of a search: its descriptor, its buffers (`bufs`: x0, x1, part0, part1, xn, logits, cache<l>), its packed
    weights and its encoder-side K/V.  `sh`: the scalars every member shares.  `ok` False: outside the limits of csrc/decode.hip
    (nothing is allocated before `fill`)."""

    def __init__(self, engine, pfx, enc_out, enc_klen, sh):
        hp = engine.hp
        Ts, B, D = enc_out.shape
        self.engine, self.pfx, self.enc_out, self.enc_klen = engine, pfx, enc_out, enc_klen
        self.bufs, self.keep = {}, []
        hs = _pick_hidden_slice(hp.ffn, B)
        self.ok = hs > 0
        if not self.ok:
            return
        beam, max_len, V, dtype = sh["beam"], sh["max_len"], sh["V"], engine.dtype
        d = self.desc = L.DecodeDesc()
        d.dtype, d.B, d.beam, d.D, d.heads, d.ffn, d.layers, d.V, d.ldv = (L.F32 if dtype == torch.float32 else L.BF16, B, beam, D, hp.heads, hp.ffn,
                                                                           hp.dec_layers, V, V)
        d.Ts, d.Tsp, d.max_len, d.min_len, d.ffn_slices, d.gelu = Ts, (Ts + 127) // 128 * 128, max_len, sh["min_len"], hp.ffn // hs, int(hp.act == "gelu")
        d.pad, d.unk, d.eos, d.step0_all_slots = sh["pad"], sh["unk"], sh["eos"], int(bool(sh["step0_all_slots"]))
        d.ln_eps, d.embed_scale = hp.ln_eps, 1.0 if hp.no_scale_embedding else float(D) ** 0.5
        d.unk_penalty, d.inv_temperature = float(sh["unk_penalty"]), 1.0 / float(sh["temperature"])
        d.diverse_groups, d.diverse_strength = int(sh.get("diverse_groups", 0)), float(sh.get("diverse_strength", 0.0))
        self.layers = (L.DecodeLayer * hp.dec_layers)()
        d.layer = ctypes.addressof(self.layers)
        self.addr = ctypes.addressof(d)
        self.ok = 0 < L.load().s2t_decode_lds_bytes(self.addr) <= LDS_CAP       # shape limits of csrc/decode.hip: checked before anything is allocated

    def fill(self):
        """buffers, packed weights and the encoder-side K/V"""
        engine, pfx, d, keep = self.engine, self.pfx, self.desc, self.keep
        hp, dev, dtype = engine.hp, engine.dev, engine.dtype
        Ts, B, D = self.enc_out.shape
        N, H, Ld, V, Tsp, FS, max_len, pad = B * d.beam, hp.heads, hp.dec_layers, d.V, d.Tsp, d.ffn_slices, d.max_len, d.pad
        lib = L.load()
        st = L.stream()

        def dev_t(shape, dt, name=None):
            t = torch.empty(shape, dtype=dt, device=dev)
            keep.append(t)
            if name:
                self.bufs[name] = t                          # by name for tools/decode_debug.py and the tests
            return t
        d.x0, d.x1 = dev_t((N, D), torch.float32, "x0").data_ptr(), dev_t((N, D), torch.float32, "x1").data_ptr()
        np_max = max(H, FS)
        d.part0, d.part1 = dev_t((np_max, N, D), dtype, "part0").data_ptr(), dev_t((np_max, N, D), dtype, "part1").data_ptr()
        d.xn = dev_t((N, D), dtype, "xn").data_ptr()
        d.logits = dev_t((N, V), torch.float32, "logits").data_ptr()
        if self.enc_klen is not None:
            keep.append(self.enc_klen)
            d.enc_klen = self.enc_klen.data_ptr()
        W, P = engine.W, engine.P
        ptr = lambda t: (keep.append(t), t.data_ptr())[1]

        def packed(name):
            """the weight in fragment-major order (s2t_decode_pack_weight): re-made per search -- the weights may have moved since the last
            one, and 52 MB of copies are tens of microseconds against a search of tens of milliseconds"""
            w = W(name)
            n, k = w.shape
            wp = dev_t(((n + 15) // 16 * 16, k), dtype)
            L.check(lib.s2t_decode_pack_weight(d.dtype, w.data_ptr(), w.stride(0), n, k, wp.data_ptr(), st), "s2t_decode_pack_weight")
            return wp.data_ptr()
        d.lnf_g, d.lnf_b = ptr(P(pfx + "layer_norm.weight")), ptr(P(pfx + "layer_norm.bias"))
        d.w_out = packed(engine.out_proj(pfx) + ".weight")
        d.embed = ptr(W(pfx + "embed_tokens.weight"))
        d.pos_table = ptr(engine.table(pad + 3 + max_len, pad))
        enc2d = self.enc_out.reshape(Ts * B, D)
        for l in range(Ld):
            lp = pfx + "layers.%d." % l
            y = self.layers[l]
            for ln, stem in (("ln1", "self_attn_layer_norm"), ("lnx", "encoder_attn_layer_norm"), ("ln2", "final_layer_norm")):
                setattr(y, ln + "_g", ptr(P(lp + stem + ".weight"))); setattr(y, ln + "_b", ptr(P(lp + stem + ".bias")))
            for f, stem in (("qkv", "self_attn.qkv"), ("o", "self_attn.out_proj"), ("xq", "encoder_attn.q_proj"),
                            ("xo", "encoder_attn.out_proj"), ("fc1", "fc1"), ("fc2", "fc2")):
                setattr(y, "w_" + f, packed(lp + stem + ".weight")); setattr(y, "b_" + f, ptr(P(lp + stem + ".bias")))
            kv = engine.linear(enc2d, lp + "encoder_attn.kv")               # [Ts * B, 2D]: the reference's static_kv, once per sentence
            kp, vp = dev_t((B, H, Tsp, 64), dtype), dev_t((B, H, 64, Tsp), dtype)      # fragment-major inside (include/s2t_hip.h)
            L.check(lib.s2t_decode_prepare_enc(d.dtype, kv.data_ptr(), kp.data_ptr(), vp.data_ptr(), Ts, Tsp, B, D, H, st), "s2t_decode_prepare_enc")
            keep.append(kv)
            y.kv_enc, y.vt_enc = kp.data_ptr(), vp.data_ptr()
            y.kv_cache = dev_t((max_len + 1, N, 2 * D), dtype, "cache%d" % l).data_ptr()


class EnsembleDecodeSession:
    """State + launch sequence of one beam search over 1..8 models that share the target dictionary (the reference's EnsembleModel,
    fairseq/sequence_generator.py:711-770).  members: [(engine, pfx, enc_out, enc_klen), ...] -- enc_out [Ts_j, B, D_j] (one column per
    SENTENCE), enc_klen int32 [B] or None; the members may differ in everything of their own (width, depth, encoder length) and must
    have one compute dtype.  The search state (records, candidates, ancestor table, step counters) exists ONCE and every member's
    descriptor names it; `members[j].bufs` / `bufs_of[j]` are member j's own buffers.  `ok` False: a member, the rules or the
    combination is refused and nothing ran.  diverse_groups G > 1: group-diverse beam search (fairseq/search.py:103-161) with
    diverse_strength >= 0, a form of the per-sentence launch (G must divide the beam; not with step0_all_slots); 0 or 1: plain.
    sampling: None, or dict(topk, topp, key) -- the sampling search (fairseq/search.py:164-278; the draw of include/s2t_hip.h
    S2TDecodeSample): forms of the per-row and per-sentence launches behind s2t_decode_step_sample / s2t_decode_graph_create_sample;
    not with diverse_groups > 1 nor step0_all_slots.  None launches exactly what was launched before.
    retain_attention (one member only; `ok` False otherwise, or when the records would pass ATTN_HIST_CAP): every hypothesis of
    `hypotheses` carries `attention`, f32 [Ts, len], the last layer's encoder attention averaged over its heads.  A member whose
    engine has `hp.layernorm_embedding` gets its decoder inputs normalised.  With neither, the session goes through the entry points
    it always used; with either, through s2t_decode_begin_ex / _step_ex / _graph_create_ex (S2TDecodeExtras).
    The other arguments as BeamDecodeSession's."""

    def __init__(self, members, beam, max_len, min_len, pad, unk, eos, V, unk_penalty=0.0, temperature=1.0, init_scores=None,
                 step0_all_slots=False, no_repeat_ngram_size=0, prefix_tokens=None, diverse_groups=0, diverse_strength=0.5, sampling=None,
                 retain_attention=False):
        members = list(members)
        assert members, "an ensemble needs at least one member"
        engine, enc_out = members[0][0], members[0][2]
        B = enc_out.shape[1]
        self.engine, self.B, self.beam, self.N, self.max_len = engine, B, beam, B * beam, max_len
        self.pad, self.eos = pad, eos
        dev = engine.dev
        N = self.N
        ngram = max(int(no_repeat_ngram_size), 0)
        self.rules, self.rules_addr = None, None                        # S2TDecodeRules when a rule beyond the descriptor's is set
        self.members = []
        self.ok = ngram != 1 and 1 <= len(members) <= 8 and all(m[0].dtype == engine.dtype and m[2].shape[1] == B for m in members)
        G, lam = int(diverse_groups), float(diverse_strength)
        if G < 0 or (G > 1 and (beam % G != 0 or not (lam >= 0.0 and math.isfinite(lam)) or step0_all_slots)):
            self.ok = False                                             # what the C ABI refuses (include/s2t_hip.h: diverse_groups)
        self.sample, self.sample_addr = None, None                      # S2TDecodeSample of a sampling search
        if sampling is not None:
            topk, topp = int(sampling.get("topk", 0)), float(sampling.get("topp", 0.0))
            if G > 1 or step0_all_slots or topk < 0 or topp != topp:
                self.ok = False                                         # (include/s2t_hip.h: s2t_decode_step_sample)
            sm = self.sample = L.DecodeSample()
            sm.topk, sm.topp, sm.key = max(topk, 0), topp, int(sampling.get("key", 0)) & 0xFFFFFFFFFFFFFFFF
            self.sample_addr = ctypes.addressof(sm)
        self.extras, self.extras_addr, self.attn_hist, self.attn_part = None, None, None, None
        self.retain_attention = bool(retain_attention)
        lne = [bool(getattr(m[0].hp, "layernorm_embedding", False)) for m in members]
        if self.retain_attention and (len(members) != 1 or (max_len + 1) * N * enc_out.shape[0] * 4 > ATTN_HIST_CAP):
            self.ok = False                                             # (include/s2t_hip.h: S2TDecodeExtras; the cap is this module's)
        if not self.ok:
            return
        sh = dict(beam=beam, max_len=max_len, min_len=min_len, pad=pad, unk=unk, eos=eos, V=V, unk_penalty=unk_penalty, temperature=temperature,
                  step0_all_slots=step0_all_slots, diverse_groups=G, diverse_strength=lam)
        for m in members:                                               # every member's limits before anything is allocated
            mem = _Member(m[0], m[1], m[2], m[3], sh)
            self.ok = mem.ok
            if not self.ok:
                return
            self.members.append(mem)
        keep = self._keep = []
        # state: one int32 and one float32 block, so that the read-back at the end is two copies
        M2 = max_len + 2
        isz = dict(tok_hist=M2 * N, par_hist=M2 * N, fin_step=B * beam, fin_row=B * beam, nfin=B, finished=B, steps=B, blacklist=N,
                   anc=N * (max_len + 1), cand_idx=N * 2 * beam)
        fsz = dict(cum_hist=M2 * N, fin_score=B * beam, cand_val=N * 2 * beam)
        self.ibuf = torch.empty((sum(isz.values()),), dtype=torch.int32, device=dev)
        self.fbuf = torch.empty((sum(fsz.values()),), dtype=torch.float32, device=dev)
        self.ioff, self.foff = {}, {}
        o = 0
        for k, n in isz.items():
            self.ioff[k] = (o, n); o += n
        o = 0
        for k, n in fsz.items():
            self.foff[k] = (o, n); o += n
        self.read_i = self.ioff["steps"][0]               # [tok_hist | par_hist | fin_step | fin_row | nfin | finished] come first
        self.read_f = self.foff["cand_val"][0]
        if init_scores is not None:
            init_scores = init_scores.to(device=dev, dtype=torch.float32).contiguous().view(-1)
            assert init_scores.numel() == N
            keep.append(init_scores)
        for mem in self.members:
            d = mem.desc
            for k, (o, n) in self.ioff.items():
                setattr(d, k, self.ibuf.data_ptr() + 4 * o)
            for k, (o, n) in self.foff.items():
                setattr(d, k, self.fbuf.data_ptr() + 4 * o)
            if init_scores is not None:
                d.init_scores = init_scores.data_ptr()
        if prefix_tokens is not None and prefix_tokens.numel() == 0:
            prefix_tokens = None
        if ngram or prefix_tokens is not None:
            r = self.rules = L.DecodeRules()
            r.no_repeat_ngram = ngram
            if prefix_tokens is not None:
                assert prefix_tokens.dim() == 2 and prefix_tokens.shape[0] == B
                self.prefix = prefix_tokens.to(device=dev, dtype=torch.int32).contiguous()
                keep.append(self.prefix)
                r.prefix_len, r.prefix = self.prefix.shape[1], self.prefix.data_ptr()
            self.rules_addr = ctypes.addressof(r)
        for mem in self.members:
            mem.fill()
        self.bufs_of = [mem.bufs for mem in self.members]
        if self.retain_attention or any(lne):
            x = self.extras = L.DecodeExtras()
            for j, mem in enumerate(self.members):
                if lne[j]:
                    g, b = mem.engine.P(mem.pfx + "layernorm_embedding.weight"), mem.engine.P(mem.pfx + "layernorm_embedding.bias")
                    keep += [g, b]
                    x.lne_g[j], x.lne_b[j] = g.data_ptr(), b.data_ptr()
            if self.retain_attention:
                d0 = self.members[0].desc
                self.attn_part = torch.empty((d0.heads, N, d0.Tsp), dtype=torch.float32, device=dev)
                self.attn_hist = torch.empty((max_len + 1, N, d0.Ts), dtype=torch.float32, device=dev)
                x.attn_part, x.attn_hist = self.attn_part.data_ptr(), self.attn_hist.data_ptr()
            self.extras_addr = ctypes.addressof(x)
        n = len(self.members)
        self.desc_array = (ctypes.c_void_p * n)(*[mem.addr for mem in self.members])     # the HOST array of descriptors of the *_ensemble calls
        self.descs_addr = ctypes.addressof(self.desc_array)
        # every member's chain up to its logits, then the shared row and sentence launches
        self.launches_per_step = sum(3 * mem.desc.layers + 2 for mem in self.members) + 2
        self.steps_run = 0

    def view_i(self, name):
        o, n = self.ioff[name]
        return self.ibuf[o:o + n]

    def view_f(self, name):
        o, n = self.foff[name]
        return self.fbuf[o:o + n]

    def run(self, bos, graph=True):
        """the whole search; returns the number of steps launched"""
        lib = L.load()
        st = L.stream()
        n = len(self.members)
        one = self.members[0].addr if n == 1 else None      # one model: the one-model entry points, as ever
        xa = self.extras_addr                               # an option of S2TDecodeExtras: the *_ex entry points for everything
        if xa:
            L.check(lib.s2t_decode_begin_ex(self.descs_addr, n, self.rules_addr, self.sample_addr, xa, int(bos), st), "s2t_decode_begin_ex")
        elif one:
            L.check(lib.s2t_decode_begin(one, int(bos), st), "s2t_decode_begin")
        else:
            L.check(lib.s2t_decode_begin_ensemble(self.descs_addr, n, int(bos), st), "s2t_decode_begin_ensemble")
        exec_ = ctypes.c_void_p(0)
        per = POLL_STEPS if graph else 1                    # steps per launch: one recorded graph holds POLL_STEPS of them
        if graph and xa:
            L.check(lib.s2t_decode_graph_create_ex(self.descs_addr, n, self.rules_addr, self.sample_addr, xa, per, ctypes.addressof(exec_)),
                    "s2t_decode_graph_create_ex")
        elif graph and self.sample_addr:
            L.check(lib.s2t_decode_graph_create_sample(self.descs_addr, n, self.rules_addr, self.sample_addr, per, ctypes.addressof(exec_)),
                    "s2t_decode_graph_create_sample")
        elif graph and not one:
            L.check(lib.s2t_decode_graph_create_ensemble(self.descs_addr, n, self.rules_addr, per, ctypes.addressof(exec_)),
                    "s2t_decode_graph_create_ensemble")
        elif graph and self.rules_addr:
            L.check(lib.s2t_decode_graph_create_rules(one, self.rules_addr, per, ctypes.addressof(exec_)), "s2t_decode_graph_create_rules")
        elif graph:
            L.check(lib.s2t_decode_graph_create(one, per, ctypes.addressof(exec_)), "s2t_decode_graph_create")
        fo, fn = self.ioff["finished"]
        finished = self.ibuf[fo:fo + fn]
        steps = 0
        try:
            while steps < self.max_len + 1:
                if graph:
                    L.check(lib.s2t_decode_graph_launch(exec_.value, st), "s2t_decode_graph_launch")
                elif xa:
                    L.check(lib.s2t_decode_step_ex(self.descs_addr, n, self.rules_addr, self.sample_addr, xa, st), "s2t_decode_step_ex")
                elif self.sample_addr:
                    L.check(lib.s2t_decode_step_sample(self.descs_addr, n, self.rules_addr, self.sample_addr, st), "s2t_decode_step_sample")
                elif not one:
                    L.check(lib.s2t_decode_step_ensemble(self.descs_addr, n, self.rules_addr, st), "s2t_decode_step_ensemble")
                elif self.rules_addr:
                    L.check(lib.s2t_decode_step_rules(one, self.rules_addr, st), "s2t_decode_step_rules")
                else:
                    L.check(lib.s2t_decode_step(one, st), "s2t_decode_step")
                steps += per                                # (the last graph may run past max_len: its kernels return at once there)
                if steps % POLL_STEPS == 0 and steps < self.max_len + 1 and bool(finished.all()):
                    break
        finally:
            if graph and exec_.value:
                torch.cuda.current_stream().synchronize()
                lib.s2t_decode_graph_destroy(exec_.value)
        steps = min(steps, self.max_len + 1)
        self.steps_run = steps
        return steps

    def hypotheses(self, normalize_scores, len_penalty):
        """Read the records back and rebuild what finalize_hypos (sequence_generator.py:502-600) collects: per sentence the
        finalised hypotheses in the order the reference appends them, each (tokens, score, positional_scores, origin)."""
        B, beam, N = self.B, self.beam, self.N
        ib = self.ibuf[:self.read_i].cpu().numpy()
        fb = self.fbuf[:self.read_f].cpu().numpy()
        iv = lambda k: ib[self.ioff[k][0]:self.ioff[k][0] + self.ioff[k][1]]
        fv = lambda k: fb[self.foff[k][0]:self.foff[k][0] + self.foff[k][1]]
        M2 = self.max_len + 2
        sent, tok, pos, score, origin, length, slots = walk_records_slots(
            iv("tok_hist").reshape(M2, N), iv("par_hist").reshape(M2, N), fv("cum_hist").reshape(M2, N), iv("nfin"),
            iv("fin_step").reshape(B, beam), iv("fin_row").reshape(B, beam), fv("fin_score").reshape(B, beam), beam, self.pad, self.eos,
            normalize_scores, len_penalty)
        dev = self.engine.dev
        tok_d, pos_d, score_d = torch.from_numpy(tok).to(dev), torch.from_numpy(pos).to(dev), torch.from_numpy(score).to(dev)
        out = [[] for _ in range(B)]
        for f in range(sent.shape[0]):
            n = int(length[f])
            out[int(sent[f])].append({"tokens": tok_d[f, :n], "score": score_d[f], "attention": None, "alignment": None,
                                      "positional_scores": pos_d[f, :n], "origin": int(origin[f]), "_score": float(score[f])})
        if self.attn_hist is not None and sent.shape[0]:
            # position p of a hypothesis was produced by step p on slot slots[f, p] of arrangement p: one gather of the records
            # (index work only, as finalize_hypos' index_select on the step route); columns past a hypothesis' length are cut off
            slots_d = torch.from_numpy(slots).to(dev)
            rec = self.attn_hist[torch.arange(slots.shape[1], device=dev)[None, :], slots_d]        # [F, Lmax, Ts]
            count = [0] * B
            for f in range(sent.shape[0]):
                s = int(sent[f])
                out[s][count[s]]["attention"] = rec[f, :int(length[f])].t()                        # src_len x tgt_len (:510-514)
                count[s] += 1
        return out


class BeamDecodeSession(EnsembleDecodeSession):
    """State + launch sequence of one beam search.  enc_out [Ts, B, D] (one column per SENTENCE), enc_klen int32 [B] or None.
    no_repeat_ngram_size: 0 (off) or >= 2 (1 is refused: `ok` False); prefix_tokens: integer [B, P], pad = free, WITHOUT EOS (the
    caller checks: sequence_generator._device_search) -- the session keeps its int32 device copy alive for the recorded graph.
    The one-member form of EnsembleDecodeSession: `desc`, `addr` and `bufs` are the member's, and `run` goes through the one-model
    entry points (s2t_decode_begin, s2t_decode_step[_rules], s2t_decode_graph_create[_rules]), or, with retain_attention or a
    --layernorm-embedding engine, through the *_ex ones."""

    def __init__(self, engine, pfx, enc_out, enc_klen, beam, max_len, min_len, pad, unk, eos, V, unk_penalty=0.0, temperature=1.0,
                 init_scores=None, step0_all_slots=False, no_repeat_ngram_size=0, prefix_tokens=None, diverse_groups=0,
                 diverse_strength=0.5, sampling=None, retain_attention=False):
        super().__init__([(engine, pfx, enc_out, enc_klen)], beam, max_len, min_len, pad, unk, eos, V, unk_penalty, temperature,
                         init_scores=init_scores, step0_all_slots=step0_all_slots, no_repeat_ngram_size=no_repeat_ngram_size,
                         prefix_tokens=prefix_tokens, diverse_groups=diverse_groups, diverse_strength=diverse_strength, sampling=sampling,
                         retain_attention=retain_attention)
        if self.members:
            m = self.members[0]
            self.desc, self.addr, self.layers = m.desc, m.addr, m.layers
        if self.ok:
            self.bufs = self.members[0].bufs


def walk_records(tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score, beam, pad, eos, normalize_scores, len_penalty):
    """walk_records_slots without the slots"""
    return walk_records_slots(tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score, beam, pad, eos, normalize_scores, len_penalty)[:6]


def walk_records_slots(tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score, beam, pad, eos, normalize_scores, len_penalty):
    """Host side of the device search (numpy): from the per-step selection records -- arrangement i = the beam after i selections:
    tok_h[i][n] the token slot n received, par_h[i][n] the slot of arrangement i-1 it continues, cum_h[i][n] its cumulative score --
    and the finalisation records (step, parent slot, score of the EOS candidate; nfin[s] of them per sentence, in the order the
    reference appends them) to what finalize_hypos builds (sequence_generator.py:502-560): tokens (ending in EOS), positional scores
    (differences of the cumulative ones), the length-normalised score (:553-554) and the step-0 slot each hypothesis descends from.
    Returns (sentence, tokens [F, Lmax] pad-filled, positional scores, score, origin, length, slots), one row per hypothesis.
    slots [F, Lmax] (0 past the length): slots[f, p] = the slot of arrangement p the hypothesis occupied when step p produced its
    token at target position p -- the final EOS comes from `fin_row` at `fin_step`, the earlier ones along `par_h` -- i.e. where the
    per-step records of that step (attn_hist[p]) hold what belongs to it."""
    B = nfin.shape[0]
    sel = np.arange(beam)[None, :] < nfin[:, None]
    sent = np.nonzero(sel)[0]
    fstep = fin_step[sel].astype(np.int64)
    rows = fin_row[sel].astype(np.int64)
    fsc = fin_score[sel].astype(np.float32)
    F = int(sent.shape[0])
    Tm = int(fstep.max()) if F else 0
    tok = np.full((F, Tm + 1), pad, dtype=np.int64)
    cum = np.zeros((F, Tm + 1), dtype=np.float32)
    idx = np.arange(F)
    slots = np.zeros((F, Tm + 1), dtype=np.int64)
    tok[idx, fstep] = eos
    cum[idx, fstep] = fsc
    slots[idx, fstep] = rows
    for i in range(Tm, 0, -1):                                         # arrangement i -> i-1 along the parent links
        act = fstep >= i
        r = rows[act]
        tok[act, i - 1] = tok_h[i][r]
        cum[act, i - 1] = cum_h[i][r]
        rows[act] = par_h[i][r]
        slots[act, i - 1] = rows[act]
    origin = rows % beam
    pos = cum.copy()
    pos[:, 1:] = cum[:, 1:] - cum[:, :-1]
    score = fsc / ((fstep + 1).astype(np.float64) ** len_penalty).astype(np.float32) if normalize_scores else fsc
    return sent, tok, pos, score.astype(np.float32), origin, fstep + 1, slots


def device_search_enabled():
    return os.environ.get("S2T_DEVICE_SEARCH", "1") != "0"
