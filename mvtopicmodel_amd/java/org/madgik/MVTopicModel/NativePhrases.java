package org.madgik.MVTopicModel;

import java.lang.reflect.Field;

/**
 * findTopicPhrases (FastQMVWVParallelTopicModel.java:1921-1976) on the GPU: the same-topic word runs of the view-0 tokens counted per
 * topic, the call that replaces lines 1555-1586 of saveTopicsandExperiment and feeds topicPhraseXMLReport.  Contract: include/mvhdp.h
 * (mvhdp_topic_phrases); equal counts come in ascending word-id order, which is this library's order, not the reference's.
 * The native lives in mvhdp_phrases_jni.cpp, built into the same libmvhdp_jni.so as NativeSampler's.
 */
public final class NativePhrases {
    static {
        System.loadLibrary("mvhdp_jni");
    }

    private NativePhrases() {}

    private static native long nTopicPhrases(long handle, int maxPerTopic, int hashBits, long[] topicOff, long[] wordOff, int[] words, int[] counts, long[] distinct, long[] occurrences, long[] sizesOut, long[] statsOut);

    /** Phrases of topic k: topicOff[k] .. topicOff[k + 1]; word ids of phrase p: words[wordOff[p] .. wordOff[p + 1]); its count: counts[p]. */
    public static final class Phrases {
        public long[] topicOff, wordOff;
        public int[] words, counts;
        public long[] distinct, occurrences;      // per topic, before the cut: keys().length and countssum (line 2037)
        public long runs, totalOccurrences, totalDistinct, kept, hashCollisions;

        /** The reference's key: the words joined by a blank. */
        public String key(int p, Object[] vocabulary) {
            StringBuilder sb = new StringBuilder();
            for (long i = wordOff[p]; i < wordOff[p + 1]; i++) {
                if (i > wordOff[p]) sb.append(' ');
                sb.append(vocabulary[words[(int) i]]);
            }
            return sb.toString();
        }

        /** count / countssum of the phrase's topic k (line 2037) */
        public double weight(int p, int k) { return (double) counts[p] / occurrences[k]; }
    }

    // NativeSampler keeps its handle private; the classes share a package and a library, not a field
    private static long handleOf(NativeSampler s) {
        try {
            Field f = NativeSampler.class.getDeclaredField("handle");
            f.setAccessible(true);
            long h = f.getLong(s);
            if (h == 0) throw new IllegalStateException("NativeSampler is closed");
            return h;
        } catch (ReflectiveOperationException e) {
            throw new IllegalStateException(e);
        }
    }

    /** maxPerTopic < 0: every phrase; saveTopicsandExperiment keeps 20 (line 1569). */
    public static Phrases topicPhrases(NativeSampler s, int numTopics, int maxPerTopic) {
        long h = handleOf(s);
        Phrases p = new Phrases();
        long[] sizes = new long[2], st = new long[5];
        nTopicPhrases(h, maxPerTopic, 0, null, null, null, null, null, null, sizes, null);
        if (sizes[0] > Integer.MAX_VALUE - 8 || sizes[1] > Integer.MAX_VALUE - 8) throw new IllegalStateException("more phrases than a Java array holds: " + sizes[0] + " / " + sizes[1]);
        p.topicOff = new long[numTopics + 1];
        p.wordOff = new long[(int) sizes[0] + 1];
        p.words = new int[(int) sizes[1]];
        p.counts = new int[(int) sizes[0]];
        p.distinct = new long[numTopics];
        p.occurrences = new long[numTopics];
        nTopicPhrases(h, maxPerTopic, 0, p.topicOff, p.wordOff, p.words, p.counts, p.distinct, p.occurrences, sizes, st);
        p.runs = st[0]; p.totalOccurrences = st[1]; p.totalDistinct = st[2]; p.kept = st[3]; p.hashCollisions = st[4];
        return p;
    }
}
