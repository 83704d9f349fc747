"""The backoff n-gram gloss model of the second pass (`sca_ngram_lm`, include/scatten.h): an ARPA
model of order 1 to 3 over the C classes, held on the device as a sorted trie and looked up in
HIP by `sca_nbest_rescore_ngram` and `sca_mwer_heads_fwd_ngram`.  The semantics are the
header's; the reference has no language model.

* `NGramLM` — the validated model: unigram arrays, bigram rows by context and trigram rows by
  bigram entry in CSR form, natural-log fp32.  Class 0 is the sentence boundary on both sides:
  `<s>` as context, `</s>` as predicted word.
* `NGramLM.from_arpa` / `.to_arpa` — standard ARPA text (log10 in the file).
* `NGramLM.from_sequences` — interpolated absolute discounting, estimated on the host in float64
  and stored in backoff form; `NGramLM.estimate` returns the float64 values themselves.
* `NGramLM.from_bigram` / `.to_bigram` — the dense `BigramLM` as an order-2 model with every
  cell explicit, and an order-1 or order-2 model as the dense table whose kernels are bitwise
  the sparse ones (the fused beam search takes the dense form only).

`rescore_nbest_device`, `Rescoring` and the steps that take one, `mwer_loss`, `MWER` and
`MWERLossOp` accept an `NGramLM` wherever they accept a `BigramLM`, except with `fusion=True`.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib as L

MAX_CLASSES = 8192  # SCA_CTC_MAX_C
MAX_ORDER = 3
LN10 = math.log(10.0)
BOS, EOS = "<s>", "</s>"


def _f32(name, a, n):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
    if a.shape != (n,) or a.dtype.kind not in "fiu":
        raise ValueError(f"NGramLM: {name} must hold {n} numbers, got shape {a.shape} of {a.dtype}")
    a = a.astype(np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"NGramLM: {name} must be finite")
    return a.astype(np.float32)


def _columns(name, grams, n, values):
    """An n-gram table as columns: `n` int64 token columns and `values` float columns.  `grams`:
    a dict {(tokens): value or (values)}, sorted here, or a tuple of `n + values` arrays in row
    order (a missing or None last value column is 0)."""
    if grams is None:
        grams = {}
    if isinstance(grams, dict):
        keys = sorted(grams)
        if any(not isinstance(k, tuple) or len(k) != n for k in keys):
            raise ValueError(f"NGramLM: the keys of {name} must be tuples of {n} class ids")
        toks = np.array(keys, np.int64).reshape(len(keys), n)
        vals = np.zeros((len(keys), values), np.float64)
        try:  # one form for every entry: a number, or a tuple of up to `values` numbers
            given = np.array([grams[k] for k in keys], np.float64).reshape(len(keys), -1)
        except ValueError:
            given = None
        if given is not None and given.shape[1] <= values:
            vals[:, :given.shape[1]] = given
        else:
            for i, k in enumerate(keys):
                v = grams[k]
                v = tuple(v) if isinstance(v, (tuple, list)) else (v,)
                if not 1 <= len(v) <= values:
                    raise ValueError(f"NGramLM: {name}[{k}] must hold 1 to {values} values, got {len(v)}")
                vals[i, :len(v)] = v
        return [toks[:, j] for j in range(n)], [vals[:, j] for j in range(values)]
    cols = list(grams)
    if len(cols) == n + values - 1 and values == 2:
        cols.append(None)
    if len(cols) != n + values:
        raise ValueError(f"NGramLM: {name} must be a dict or {n + values} arrays, got {len(cols)}")
    toks = [np.asarray(c.detach().cpu() if torch.is_tensor(c) else c) for c in cols[:n]]
    rows = toks[0].shape[0] if toks[0].ndim == 1 else -1
    for t in toks:
        if t.ndim != 1 or t.shape[0] != rows or t.dtype.kind not in "iu":
            raise ValueError(f"NGramLM: the token columns of {name} must be integer arrays of one length")
    vals = [np.zeros(rows) if c is None else np.asarray(c.detach().cpu() if torch.is_tensor(c) else c, np.float64)
            for c in cols[n:]]
    if any(v.shape != (rows,) for v in vals):
        raise ValueError(f"NGramLM: the value columns of {name} must have the token columns' length {rows}")
    return [t.astype(np.int64) for t in toks], vals


class NGramLM:
    """A backoff n-gram gloss model of `order` 1 to 3 over `num_classes` classes: `uni_lp`,
    `uni_bo` (C) (natural-log probabilities and backoff weights; `uni_bo` may be None with order
    1), `bigrams` {(v, w): (lp, bo)} — or {(v, w): lp}, or arrays (v, w, lp, bo) in row order —
    and `trigrams` {(u, v, w): lp} or arrays (u, v, w, lp).  Class 0 is the sentence boundary:
    `<s>` as context and `</s>` as predicted word, so `uni_lp[0]` is p(</s>), `uni_bo[0]` the
    backoff weight of <s>, and lm(empty) = p(0 | 0).  The score of a labelling follows the ARPA
    backoff rule (include/scatten.h).

    Validated on the host: finite values, tokens in [0, C), no trigram with 0 in the middle (0 is
    `u` only at the sentence start and `w` only at its end), every trigram's (u, v) stored as a
    bigram, rows sorted and unique (arrays; a dict is sorted here), nothing above `order`.  The
    trie tensors are built once, fp32 / int32 on `device` (default: the host, until
    `.to(device)`)."""

    def __init__(self, order, num_classes, uni_lp, uni_bo=None, bigrams=None, trigrams=None, device=None):
        if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order must be an int in [1, {MAX_ORDER}], got {order!r}")
        C = int(num_classes)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"NGramLM: num_classes must lie in [1, {MAX_CLASSES}], got {num_classes}")
        t = {"uni_lp": _f32("uni_lp", uni_lp, C),
             "uni_bo": np.zeros(C, np.float32) if uni_bo is None else _f32("uni_bo", uni_bo, C)}
        (bv, bw), (blp, bbo) = _columns("bigrams", bigrams, 2, 2)
        (tu, tv, tw), (tlp,) = _columns("trigrams", trigrams, 3, 1)
        if (order < 2 and len(bv)) or (order < 3 and len(tu)):
            raise ValueError(f"NGramLM: an order-{order} model takes no n-grams above its order")
        for name, cols in (("bigrams", (bv, bw)), ("trigrams", (tu, tv, tw))):
            for c in cols:
                if len(c) and (c.min() < 0 or c.max() >= C):
                    raise ValueError(f"NGramLM: the tokens of {name} must lie in [0, {C})")
        if len(tv) and (tv == 0).any():
            raise ValueError("NGramLM: a trigram (u, 0, w) has the sentence boundary inside it: 0 may be u only at "
                             "the sentence start and w only at its end")
        bkey, tkey = bv * C + bw, (tu * C + tv) * C + tw
        for name, key in (("bigrams", bkey), ("trigrams", tkey)):
            if len(key) > 1 and not (np.diff(key) > 0).all():
                raise ValueError(f"NGramLM: the rows of {name} must be sorted by (context, word) and unique")
        entry = np.searchsorted(bkey, tu * C + tv)  # the bigram entry of every trigram's context
        if len(tu) and not (len(bkey) and (bkey[np.minimum(entry, len(bkey) - 1)] == tu * C + tv).all()):
            raise ValueError("NGramLM: every trigram's context (u, v) must be stored as a bigram")
        n_bi, n_tri = len(bkey), len(tkey)
        t["bi_ptr"] = np.searchsorted(bv, np.arange(C + 1)).astype(np.int32)
        t["bi_tok"] = bw.astype(np.int32)
        t["bi_lp"], t["bi_bo"] = _f32("the bigrams' lp", blp, n_bi), _f32("the bigrams' bo", bbo, n_bi)
        t["tri_ptr"] = np.searchsorted(entry, np.arange(n_bi + 1)).astype(np.int32)
        t["tri_tok"] = tw.astype(np.int32)
        t["tri_lp"] = _f32("the trigrams' lp", tlp, n_tri)
        self._set(order, C, {k: torch.from_numpy(v).to(device) for k, v in t.items()})
        self.skipped = 0

    def _set(self, order, C, tensors):
        self.order, self._C, self.tensors = order, C, tensors
        for k, v in tensors.items():
            setattr(self, k, v)
        s = L.NgramLm(order=order, C=C, n_bi=self.bi_tok.numel(), n_tri=self.tri_tok.numel())
        for k, v in tensors.items():
            setattr(s, k, v.data_ptr() if v.numel() else None)
        self.struct = s  # sca_ngram_lm: the pointers of `tensors`, which this object keeps alive

    @property
    def num_classes(self):
        return self._C

    @property
    def device(self):
        return self.uni_lp.device

    @property
    def num_entries(self):
        """(unigrams, bigrams, trigrams) stored."""
        return self._C, self.bi_tok.numel(), self.tri_tok.numel()

    @property
    def nbytes(self):
        """The bytes of the trie's tensors."""
        return sum(v.numel() * v.element_size() for v in self.tensors.values())

    def to(self, device):
        lm = object.__new__(NGramLM)
        lm._set(self.order, self._C, {k: v.to(device) for k, v in self.tensors.items()})
        lm.skipped = self.skipped
        return lm

    def __repr__(self):
        _, nb, nt = self.num_entries
        return f"NGramLM(order={self.order}, C={self._C}, bigrams={nb}, trigrams={nt}, device={self.device})"

    # ------------------------------------------------------------------ host views
    def bigram_dict(self):
        """{(v, w): (lp, bo)} of the stored bigrams (host floats of the fp32 values)."""
        ptr, tok = self.bi_ptr.cpu().numpy(), self.bi_tok.cpu().numpy()
        lp, bo = self.bi_lp.cpu().numpy(), self.bi_bo.cpu().numpy()
        ctx = np.repeat(np.arange(self._C), np.diff(ptr))
        return {(int(v), int(w)): (float(a), float(b)) for v, w, a, b in zip(ctx, tok, lp, bo)}

    def trigram_dict(self):
        """{(u, v, w): lp} of the stored trigrams."""
        bptr, btok = self.bi_ptr.cpu().numpy(), self.bi_tok.cpu().numpy()
        ctx = np.repeat(np.arange(self._C), np.diff(bptr))
        tptr, ttok, lp = self.tri_ptr.cpu().numpy(), self.tri_tok.cpu().numpy(), self.tri_lp.cpu().numpy()
        ent = np.repeat(np.arange(len(btok)), np.diff(tptr))
        return {(int(ctx[e]), int(btok[e]), int(w)): float(a) for e, w, a in zip(ent, ttok, lp)}

    # ------------------------------------------------------------------ the dense form
    @classmethod
    def from_bigram(cls, bigram_lm):
        """The dense `BigramLM` as an order-2 model with all C * C cells explicit (the unigram
        arrays are 0 and never read), on the table's device."""
        table = bigram_lm.table
        C = table.shape[0]
        ids = np.arange(C, dtype=np.int64)
        flat = table.detach().cpu().numpy().reshape(-1)
        return cls(2, C, np.zeros(C, np.float32), None, (np.repeat(ids, C), np.tile(ids, C), flat, None),
                   device=table.device)

    def to_bigram(self):
        """The dense `BigramLM` of an order-1 or order-2 model, on its device: a stored cell holds
        its value, a backed-off one fp32(uni_bo[v] + uni_lp[w]), so the dense kernels on it are
        bitwise the sparse ones; with order 1 every row is `uni_lp`.  This is the form the fused
        beam search takes (shallow fusion)."""
        from .nbest import BigramLM
        if self.order > 2:
            raise ValueError("NGramLM.to_bigram: only a model of order 1 or 2 has a dense bigram form")
        lp, bo = self.uni_lp.cpu().numpy(), self.uni_bo.cpu().numpy()
        if self.order == 1:
            table = np.tile(lp, (self._C, 1))
        else:
            table = bo[:, None] + lp[None, :]  # fp32 + fp32, the device's addition
            ctx = np.repeat(np.arange(self._C), np.diff(self.bi_ptr.cpu().numpy()))
            table[ctx, self.bi_tok.cpu().numpy()] = self.bi_lp.cpu().numpy()
        return BigramLM(torch.from_numpy(np.ascontiguousarray(table, np.float32)), self.device)

    # ------------------------------------------------------------------ estimation
    @staticmethod
    def estimate(seqs, num_classes, order=3, discount=0.75, add_k=1.0):
        """The float64 estimate behind `from_sequences`: {"uni_lp", "uni_bo" (C) float64,
        "bigrams" {(v, w): (lp, bo)}, "trigrams" {(u, v, w): lp}}, natural log.  Interpolated
        absolute discounting in backoff form over path = [0] + seq + [0]:
          p1(w) = (c(w) + k) / (N + k C), </s> counted and <s> not
          p_n(w | ctx) = max(c(ctx, w) - D, 0) / c(ctx) + gamma(ctx) p_{n-1}(w | ctx'),
          gamma(ctx) = D N1+(ctx .) / c(ctx)
        Every seen n-gram is stored with its interpolated value and bo(ctx) = log gamma(ctx); an
        unseen context has no entries and backoff weight 0, so every conditional distribution
        sums to 1."""
        C, D, k = int(num_classes), float(discount), float(add_k)
        if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order must be an int in [1, {MAX_ORDER}], got {order!r}")
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"NGramLM: num_classes must lie in [1, {MAX_CLASSES}], got {num_classes}")
        if not (math.isfinite(k) and k > 0.0):
            raise ValueError(f"NGramLM: add_k must be finite and positive, got {add_k!r}")
        if not 0.0 < D < 1.0:
            raise ValueError(f"NGramLM: discount must lie in (0, 1), got {discount!r}")
        c1 = np.zeros(C, np.float64)
        c2, c3 = collections.Counter(), collections.Counter()
        for seq in seqs:
            ids = [int(v) for v in seq]
            if any(not 1 <= v < C for v in ids):
                raise ValueError(f"NGramLM: tokens must lie in [1, {C}) (0 is the sentence boundary), got {ids}")
            path = [0] + ids + [0]
            for i in range(1, len(path)):
                c1[path[i]] += 1
                c2[path[i - 1], path[i]] += 1
                if i >= 2:
                    c3[path[i - 2], path[i - 1], path[i]] += 1
        p1 = (c1 + k) / (c1.sum() + k * C)
        out = {"uni_lp": np.log(p1), "uni_bo": np.zeros(C, np.float64), "bigrams": {}, "trigrams": {}}
        if order >= 2:
            ctx_n, ctx_types = collections.Counter(), collections.Counter()
            for (v, w), n in c2.items():
                ctx_n[v] += n
                ctx_types[v] += 1
            for v, n in ctx_n.items():
                out["uni_bo"][v] = math.log(D * ctx_types[v] / n)
            p2 = {(v, w): (n - D) / ctx_n[v] + D * ctx_types[v] / ctx_n[v] * p1[w] for (v, w), n in c2.items()}
            ctx3_n, ctx3_types = collections.Counter(), collections.Counter()
            if order >= 3:
                for (u, v, w), n in c3.items():
                    ctx3_n[u, v] += n
                    ctx3_types[u, v] += 1
                out["trigrams"] = {(u, v, w): math.log((n - D) / ctx3_n[u, v] +
                                                       D * ctx3_types[u, v] / ctx3_n[u, v] * p2[v, w])
                                   for (u, v, w), n in c3.items()}
            out["bigrams"] = {vw: (math.log(p), math.log(D * ctx3_types[vw] / ctx3_n[vw]) if vw in ctx3_n else 0.0)
                              for vw, p in p2.items()}
        return out

    @classmethod
    def from_sequences(cls, seqs, num_classes, order=3, discount=0.75, add_k=1.0, device=None):
        """`estimate` on token-id sequences (host-side numpy float64), cast to fp32 once."""
        e = cls.estimate(seqs, num_classes, order, discount, add_k)
        return cls(order, num_classes, e["uni_lp"], e["uni_bo"], e["bigrams"] or None, e["trigrams"] or None, device)

    # ------------------------------------------------------------------ ARPA text
    @classmethod
    def from_arpa(cls, path_or_text, vocab, num_classes=None, device=None):
        """A model from standard ARPA text (a path, or the text itself: anything with a line
        break): log10 in the file, natural log in memory.  `vocab` maps gloss strings to class ids
        in [1, C), C = `num_classes` (default: the largest id + 1); `<s>` and `</s>` map to 0:
        `uni_lp[0]` comes from `</s>`, `uni_bo[0]` from `<s>`.  N-grams with a word outside
        `vocab`, with `<s>` or `</s>` where a sentence has none, or (trigrams) whose context is
        not a stored bigram are skipped and counted in `.skipped`.  A class without a unigram gets
        the `<unk>` value if the file has one, else the smallest unigram value, and backoff
        weight 0.  Orders above 3 raise ValueError."""
        text = path_or_text
        if not (isinstance(text, str) and "\n" in text):
            with open(os.fspath(path_or_text), encoding="utf-8") as fh:
                text = fh.read()
        vocab = dict(vocab)
        if any(isinstance(i, bool) or not isinstance(i, int) or i < 1 for i in vocab.values()) or \
                len(set(vocab.values())) != len(vocab):
            raise ValueError("NGramLM.from_arpa: vocab must map gloss strings to distinct class ids >= 1")
        C = int(num_classes) if num_classes is not None else max(vocab.values(), default=0) + 1
        if not 1 <= C <= MAX_CLASSES or any(i >= C for i in vocab.values()):
            raise ValueError(f"NGramLM.from_arpa: class ids must lie in [1, C = {C}), C <= {MAX_CLASSES}")
        grams = {1: {}, 2: {}, 3: {}}
        section, top, skipped, unk = 0, 0, 0, None
        for raw in text.splitlines():
            line = raw.strip()
            if not line or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("ngram "):
                n, _, count = line[6:].partition("=")
                if int(n) > MAX_ORDER and int(count) > 0:
                    raise ValueError(f"NGramLM.from_arpa: order {int(n)} is above {MAX_ORDER}")
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-7])
                if section > MAX_ORDER:
                    raise ValueError(f"NGramLM.from_arpa: order {section} is above {MAX_ORDER}")
                top = max(top, section)
                continue
            if section == 0:
                continue  # a header comment
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"NGramLM.from_arpa: cannot read the {section}-gram line {raw!r}")
            lp = float(f[0]) * LN10
            bo = float(f[section + 1]) * LN10 if len(f) == section + 2 else 0.0
            words = f[1:section + 1]
            if section == 1 and words[0] in (BOS, EOS, "<unk>"):
                if words[0] == "<unk>":
                    unk = lp
                    skipped += "<unk>" not in vocab
                    if "<unk>" not in vocab:
                        continue
                else:
                    grams[1][words[0]] = (lp, bo)
                    continue
            ids = []
            for j, w in enumerate(words):
                if w == BOS:
                    ids.append(0 if (j == 0 and section > 1) else None)
                elif w == EOS:
                    ids.append(0 if j == section - 1 else None)
                else:
                    ids.append(vocab.get(w))
            if None in ids or (section == 3 and ids[1] == 0):
                skipped += 1
                continue
            grams[section][tuple(ids)] = (lp, bo)
        if top == 0:
            raise ValueError("NGramLM.from_arpa: no \\1-grams: section found")
        uni = grams[1]
        stored = [v[0] for v in uni.values()]
        if not stored:
            raise ValueError("NGramLM.from_arpa: no unigram of the vocabulary or </s> found")
        floor = unk if unk is not None else min(stored)
        uni_lp, uni_bo = np.full(C, floor, np.float64), np.zeros(C, np.float64)
        for key, (lp, bo) in uni.items():
            if key == BOS:
                uni_bo[0] = bo
            elif key == EOS:
                uni_lp[0] = lp
            else:
                uni_lp[key[0]], uni_bo[key[0]] = lp, bo
        tri = {}
        for key, (lp, _) in grams[3].items():
            if key[:2] in grams[2]:
                tri[key] = lp
            else:
                skipped += 1
        lm = cls(top, C, uni_lp, uni_bo, grams[2] or None, tri or None, device)
        lm.skipped = skipped
        return lm

    def to_arpa(self, vocab):
        """The model as ARPA text (log10, 9 significant digits).  `vocab` maps gloss strings to
        class ids and must name every class in [1, C)."""
        word = {i: w for w, i in dict(vocab).items()}
        if any(c not in word for c in range(1, self._C)):
            raise ValueError(f"NGramLM.to_arpa: vocab must name every class in [1, {self._C})")

        def num(v):
            return "%.9g" % (float(v) / LN10)

        def ctx(c):
            return BOS if c == 0 else word[c]

        def last(c):
            return EOS if c == 0 else word[c]

        lp, bo = self.uni_lp.cpu().numpy(), self.uni_bo.cpu().numpy()
        bi = self.bigram_dict() if self.order >= 2 else {}
        tri = self.trigram_dict() if self.order >= 3 else {}
        counts = [self._C + 1, len(bi), len(tri)][:self.order]
        lines = ["\\data\\"] + [f"ngram {n + 1}={c}" for n, c in enumerate(counts)] + ["", "\\1-grams:"]
        tail = (lambda b: "\t" + num(b)) if self.order >= 2 else (lambda b: "")
        lines += [f"-99\t{BOS}" + tail(bo[0]), f"{num(lp[0])}\t{EOS}"]
        lines += [f"{num(lp[c])}\t{word[c]}" + tail(bo[c]) for c in range(1, self._C)]
        if self.order >= 2:
            tail = (lambda b: "\t" + num(b)) if self.order >= 3 else (lambda b: "")
            lines += ["", "\\2-grams:"] + [f"{num(a)}\t{ctx(v)} {last(w)}" + tail(b) for (v, w), (a, b) in bi.items()]
        if self.order >= 3:
            lines += ["", "\\3-grams:"] + [f"{num(a)}\t{ctx(u)} {word[v]} {last(w)}" for (u, v, w), a in tri.items()]
        return "\n".join(lines + ["", "\\end\\", ""])


__all__ = ["NGramLM", "MAX_ORDER"]
