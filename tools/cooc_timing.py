"""Cost of mvhdp_word_cooccurrence at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then
the calls, each beside the host route it replaces.  Writes a markdown report (default profiles/word_cooccurrence.md).

  timeout -k 10 1100 python tools/cooc_timing.py [--workload C4] [--docs D] [--sweeps 25] [--host-docs 16384] [--out profiles/word_cooccurrence.md]

  (i)   view 0, the top 20 words of every topic, window 0, 10 and 110
  (ii)  view 1, the top 20 items of every topic, window 0
  (iii) view 0, the top 64 words of every topic, window 10
  (iv)  a caller's corpus: the first 65 536 documents of view 0 handed in as host arrays, window 10
Wall times are host clocks around the synchronous call: three calls, the median of the last two; stats.kernel_ms is the stream's own time.
The host route is the contract vectorised with numpy on at most 16 threads, from tokens that are on the host already: per chunk of entities
the positions that hit a set are spread over the windows that hold them, made unique per (window, word), expanded to slots and to pairs of
slots of one set, and counted with np.bincount.  It runs on the first --host-docs entities only (minutes otherwise), is compared there
with the device's answer for the same range, cell by cell, and its time is scaled by the positions read.
Atomics: a document-mode call adds 1 per pair of present slots per entity and set, so the adds issued are the sum of co; a sliding call
adds once per chunk of 64 window starts, entity, set and pair that overlaps, which the host route bounds from above on its entities by the
sum of (present slots)^2 per (entity, chunk, set)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault("OMP_NUM_THREADS", "16")                               # the host baselines: at most 16 threads
if int(os.environ["OMP_NUM_THREADS"]) > 16:
    os.environ["OMP_NUM_THREADS"] = "16"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, resource_lines, timed, trained_sampler  # noqa: E402

THREADS = 16
CALLER_DOCS = 65536
EXPANDED = 4_000_000                                                         # (position, window) pairs of one host chunk, about


def index_of(sets, V):
    """wid [V]: the word's place among the listed words or -1; first [U + 1] and slot: word u sits in the flat slots slot[first[u] .. first[u + 1])"""
    S, n = sets.shape
    flat = np.flatnonzero(sets.reshape(-1) >= 0)
    types = sets.reshape(-1)[flat]
    o = np.argsort(types, kind="stable")
    words, counts = np.unique(types[o], return_counts=True)
    wid = np.full(V, -1, dtype=np.int64)
    wid[words] = np.arange(len(words))
    return wid, np.concatenate([[0], np.cumsum(counts)]), flat[o].astype(np.int64)


def runs(count):
    """for groups of the given sizes laid end to end: (index of every (member, member) pair's first, of its second)"""
    start = np.cumsum(count) - count
    begin, size = np.repeat(start, count), np.repeat(count, count)
    a = np.repeat(np.arange(int(count.sum())), size)
    b = begin[a] + np.arange(len(a)) - np.repeat(np.cumsum(size) - size, size)
    return a, b


def host_chunk(off, tok, lo, hi, W, V, n, cells, wid, first, slot):
    """(co flat, windows, the bound on the adds of a sliding call) of the entities [lo, hi)"""
    t = tok[off[lo]:off[hi]].astype(np.int64)
    L = np.diff(off[lo:hi + 1])
    slide = (L > W) if W > 0 else np.zeros(len(L), dtype=bool)
    nwin = np.where(L == 0, 0, np.where(slide, L - W + 1, 1))
    base = np.cumsum(nwin) - nwin
    doc = np.repeat(np.arange(len(L)), L)
    p = np.arange(len(t)) - np.repeat(off[lo:hi] - off[lo], L)
    u = np.where(t < V, wid[np.minimum(t, V - 1)], -1)
    hit = u >= 0
    doc, p, u = doc[hit], p[hit], u[hit]
    s = slide[doc]
    w_lo = np.where(s, np.maximum(p - W + 1, 0), 0)
    w_hi = np.where(s, np.minimum(p, L[doc] - W), 0)
    cnt = w_hi - w_lo + 1
    win = np.repeat(base[doc] + w_lo, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    key = np.unique(win * len(first) + np.repeat(u, cnt))                    # (window, word) present
    win, u = key // len(first), key % len(first)
    m = first[u + 1] - first[u]
    sl = slot[np.repeat(first[u], m) + np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)]
    win = np.repeat(win, m)
    o = np.lexsort((sl, win))
    win, sl = win[o], sl[o]
    st = sl // n
    new = np.r_[True, (win[1:] != win[:-1]) | (st[1:] != st[:-1])] if len(win) else np.zeros(0, dtype=bool)
    count = np.diff(np.r_[np.flatnonzero(new), len(win)])
    a, b = runs(count)
    co = np.bincount(sl[a] * n + sl[b] % n, minlength=cells)
    # the adds of a sliding call: present slots per (entity, chunk of 64 starts, set), squared
    wdoc = np.repeat(np.arange(len(L)), nwin)
    chunk = (win - base[wdoc[win]]) // 64 if len(win) else win
    k = np.unique((wdoc[win] * (int(nwin.max(initial=1)) // 64 + 1) + chunk) * (cells // n) + sl) if len(win) else win
    g = np.unique(k // n, return_counts=True)[1] if len(k) else k
    return co, int(nwin.sum()), int((g.astype(np.int64) ** 2).sum())


def host_route(off, tok, sets, V, W, docs):
    """the first `docs` entities: (co, windows, adds bound, ms)"""
    S, n = sets.shape
    wid, first, slot = index_of(sets, V)
    t0 = time.perf_counter()
    per = max(16, int(EXPANDED // (max(W, 1) * max(1.0, off[docs] / max(docs, 1)))))
    cuts = list(range(0, docs, per)) + [docs]
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda c: host_chunk(off, tok, c[0], c[1], W, V, n, S * n * n, wid, first, slot), zip(cuts[:-1], cuts[1:])))
    co = np.sum([p[0] for p in parts], axis=0).reshape(S, n, n)
    return co, sum(p[1] for p in parts), sum(p[2] for p in parts), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--host-docs", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_cooccurrence.md"))
    args = ap.parse_args()
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V = s.K, s.V
    H = min(args.host_docs, D)
    lines = ["# mvhdp_word_cooccurrence: timings", "",
             f"Written by tools/cooc_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities, {[int(corpus.doc_off[m][-1]) for m in range(len(V))]} tokens per view; the random start of bench.py, then "
             f"{args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1; kernel_ms: the stream's time over the kernels.  "
             f"Host route: the contract vectorised with numpy on {THREADS} threads from tokens on the host, run on the first {H} entities, compared there with the "
             "device's counts cell by cell, and scaled by the positions read.", ""]
    slower = []

    def report(name, m, sets, W, corpus_arg=None, docs=None):
        off, tok = corpus.doc_off[m], corpus.tokens[m]
        n_docs = D if docs is None else docs
        first, med, r = timed(lambda: s.word_cooccurrence(sets, m, W, corpus=corpus_arg))
        h = min(H, n_docs)
        co, windows, bound, ms = host_route(off, tok, sets, V[m], W, h)
        part = s.word_cooccurrence(sets, m, W, 0, h, corpus=corpus_arg)
        same = bool(np.array_equal(part.co, co)) and part.windows == windows
        host = ms * r.stats.tokens / max(part.stats.tokens, 1)
        st = r.stats
        if W == 0:
            adds = int(r.co.sum())
            how = f"{adds} adds issued"
        else:
            adds = int(bound * st.tokens / max(part.stats.tokens, 1))
            how = f"at most {adds} adds issued (the bound of the host's entities, scaled)"
        line = (f"- {name}: {med:.1f} ms a call (first call {first:.1f} ms, kernel_ms {st.kernel_ms:.1f}); {r.windows} windows, {st.tokens} positions, {st.hits} hits "
                f"({100.0 * st.hits / max(st.tokens, 1):.0f} %), {st.distinct_words} distinct words in {st.memberships} slots; {how}: {adds / max(st.tokens, 1):.2f} a position, "
                f"{adds / max(st.kernel_ms, 1e-9) / 1e6:.2f} G adds/s over kernel_ms; host route: {ms:.0f} ms on {h} entities ({'equal' if same else 'DIFFERENT'} counts), "
                f"scaled {host:.0f} ms = {host / med:.1f} x the call")
        lines.append(line)
        print(line, file=sys.stderr, flush=True)
        if med >= host:
            slower.append(name)
        if not same:
            raise SystemExit("the host route and the device disagree: " + name)

    top20 = s.top_words(0, 20)[0]
    for W in (0, 10, 110):
        report(f"(i) view 0 ({V[0]} types), the top 20 words of {K} topics, window {W}", 0, top20, W)
    report(f"(ii) view 1 ({V[1]} types), the top 20 items of {K} topics, window 0", 1, s.top_words(1, 20)[0], 0)
    report(f"(iii) view 0, the top 64 words of {K} topics, window 10", 0, s.top_words(0, 64)[0], 10)
    nc = min(CALLER_DOCS, D)
    off0 = corpus.doc_off[0][:nc + 1]
    report(f"(iv) a caller's corpus of {nc} documents ({int(off0[-1])} tokens of view 0, from the host), the top 20 words, window 10", 0, top20, 10,
           corpus_arg=(off0, corpus.tokens[0][:int(off0[-1])]), docs=nc)
    s.close()
    lines += ["", "Slower than its host route: " + (", ".join(slower) if slower else "none"), "", "## the kernel as compiled", ""]
    lines += ["- " + l for l in resource_lines("mvhdp_cooc.hip", r"cooc_kernel")] + [""]
    lines += ["## Reading the numbers", "",
              "- The per-wave state of a document-mode call at 400 sets is in LDS; with a sliding span and n = 20 the coverage words "
              "(`cov[n_sets][n]`, 64 KB a wave) do not fit and sit in a per-wave slice of global memory, written by device-scope atomics.  That, "
              "and a fence and a pass over the touched sets per chunk of 64 window starts, is what a sliding call costs over a document-mode one; "
              "coverage words in LDS keyed by the touched sets of a chunk were not tried.",
              "- The adds into `co` are 64-bit device-scope atomics, one per pair of present slots per entity (document mode) or per chunk (sliding); what shares a cell "
              "inside an entity is combined in the wave (the popcount), what shares it across entities is not: the head words' cells stay hot at the L2.",
              "- Wall time minus kernel_ms is the host side of a call: the index build, the entities' order (a counting sort), the allocations and the copy of `co`.", "",
              "## Not done", "",
              "- A JNI class (the shim's class table is pinned by a test).",
              "- A `mvhdp_group_*` C form over rank processes: each rank calls its own handle and the host sums (`merge_word_cooccurrence`).",
              "- C_V's indirect cosine confirmation, which the host can form from `co`.",
              "- Windows restricted by assignment: `mvhdp_diagnostics` keeps that.",
              "- Weighted tokens.",
              "- Splitting one very long entity over several waves; combining the hot cells of `co` across the entities of a block.", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
