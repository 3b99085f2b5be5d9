"""findTopicPhrases (FastQMVWVParallelTopicModel.java:1921-1976) restated: the literal three-branch loop over the positions of every
entity's view-0 span, a dictionary per topic, then the order and the cut of include/mvhdp.h (count descending, equal counts by word-id
sequence ascending with a proper prefix first) and the merge of document shards.  Plain Python on purpose: it shares nothing with the
device's derivation (no runs, no scan, no hash)."""
import numpy as np


def find_topic_phrases(K, doc_off, tokens, z):
    """phrases[k] = {word-id tuple: count}, the reference's TObjectIntHashMap per topic"""
    phrases = [dict() for _ in range(K)]
    doc_off = [int(x) for x in doc_off]
    tokens = [int(x) for x in tokens]
    z = [int(x) for x in z]
    for d in range(len(doc_off) - 1):
        prevtopic = prevfeature = -1
        sb = None
        for pi in range(doc_off[d], doc_off[d + 1]):
            feature, topic = tokens[pi], z[pi]
            if topic == prevtopic:                                           # same topic: start [prevfeature, feature] or append
                if sb is None:
                    sb = [prevfeature, feature]
                else:
                    sb.append(feature)
            elif sb is not None:                                             # break: count, back to EMPTY; this token is swallowed
                key = tuple(sb)
                phrases[prevtopic][key] = phrases[prevtopic].get(key, 0) + 1
                prevtopic = prevfeature = -1
                sb = None
            else:                                                            # hold
                prevtopic, prevfeature = topic, feature
        # nothing is flushed at the end of the entity
    return phrases


def order_and_cut(table, max_per_topic):
    """[(ids, count)] of one topic's {ids: count}: count descending, then the id sequence ascending (Python's tuple order puts a proper
    prefix first), cut at max_per_topic (< 0: no cut)"""
    out = sorted(table.items(), key=lambda e: (-e[1], e[0]))
    return out if max_per_topic < 0 else out[:max_per_topic]


def arrays(phrases, max_per_topic):
    """what mvhdp_topic_phrases returns: topic_off, word_off, words, counts, distinct, occurrences"""
    K = len(phrases)
    topic_off, word_off, words, counts = [0], [0], [], []
    for k in range(K):
        for ids, c in order_and_cut(phrases[k], max_per_topic):
            words.extend(ids)
            word_off.append(len(words))
            counts.append(c)
        topic_off.append(len(counts))
    return (np.array(topic_off, np.int64), np.array(word_off, np.int64), np.array(words, np.int32), np.array(counts, np.int32),
            np.array([len(p) for p in phrases], np.int64), np.array([sum(p.values()) for p in phrases], np.int64))


def topic_phrases(K, doc_off, tokens, z, max_per_topic):
    return arrays(find_topic_phrases(K, doc_off, tokens, z), max_per_topic)


def lists(phrases, max_per_topic):
    """[[(ids, count), ...] per topic], the shape of TopicPhrases.phrases"""
    return [order_and_cut(p, max_per_topic) for p in phrases]


def merge(shard_phrases, max_per_topic):
    """the per-topic dictionaries of several shards summed key by key, then ordered and cut"""
    K = len(shard_phrases[0])
    out = [dict() for _ in range(K)]
    for sp in shard_phrases:
        for k in range(K):
            for ids, c in sp[k].items():
                out[k][ids] = out[k].get(ids, 0) + c
    return out, lists(out, max_per_topic)


def count_runs(doc_off, z):
    """maximal same-topic runs over all spans (mvhdp_phrase_stats.runs)"""
    z = np.asarray(z)
    n = 0
    for d in range(len(doc_off) - 1):
        s = z[int(doc_off[d]):int(doc_off[d + 1])]
        if len(s):
            n += 1 + int((s[1:] != s[:-1]).sum())
    return n
