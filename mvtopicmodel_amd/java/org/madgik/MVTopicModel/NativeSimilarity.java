package org.madgik.MVTopicModel;

import java.lang.reflect.Field;
import java.util.Arrays;

/**
 * What SciTopicFlow does with a trained model (SciTopicFlow.java:246-260), on the GPU: the thresholded topic lists of saveTopicsPerDoc,
 * their sums per author / project / venue (CalcEntityTopicDistributionsAndTrends) and the all-pairs similarities of calcSimilarities /
 * CalcTopicSimilarities.  Contracts: include/mvhdp.h (mvhdp_doc_topics_top, mvhdp_entity_topic_distributions, mvhdp_similar_pairs).
 * The natives live in mvhdp_sim_jni.cpp, built into the same libmvhdp_jni.so as NativeSampler's.
 */
public final class NativeSimilarity {
    static {
        System.loadLibrary("mvhdp_jni");
    }

    public static final int COS_FOLDED = 0;   // 1 - |1 - cos|: calcSimilarities (SciTopicFlow.java:1483)
    public static final int COS = 1;          // cos: CalcTopicSimilarities (SciTopicFlow.java:1144)
    public static final int JSD = 2;          // Maths.jensenShannonDivergence (SciTopicFlow.java:1461)

    private NativeSimilarity() {}

    private static native long nSimilarPairs(long handle, int metric, int n, int dim, double[] xFlat, double minWeight, double threshold, int stripeRows, long candidateCapacity, int[] i, int[] j, double[] sim, long[] statsOut, double[] marginOut);
    private static native long nDocTopicsTop(long handle, double[] viewWeights, long d0, long d1, double threshold, int max, long[] rowOff, int[] topics, double[] weights);
    private static native void nEntityTopicDistributions(long handle, double[] viewWeights, double threshold, int max, int roundDigits, long[] memberOff, long[] members, double[] out);

    /** The pairs i < j with sim > threshold, sorted by (i, j); sim unrounded (round3 is the flow's rounding). */
    public static final class Pairs {
        public int[] i, j;
        public double[] sim;
        public long pairsScreened, candidates, emitted;
        public int stripes, regrown;
        public double margin;
    }

    /** The topic lists of entities [d0, d1): topics / weights of entity d at rowOff[d - d0] .. rowOff[d - d0 + 1]. */
    public static final class TopicLists {
        public long[] rowOff;
        public int[] topics;
        public double[] weights;
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

    public static Pairs similarPairs(NativeSampler s, int metric, int n, int dim, double[] xFlat, double minWeight, double threshold) {
        return similarPairs(s, metric, n, dim, xFlat, minWeight, threshold, 0, 0L);
    }

    public static Pairs similarPairs(NativeSampler s, int metric, int n, int dim, double[] xFlat, double minWeight, double threshold, int stripeRows, long candidateCapacity) {
        long h = handleOf(s);
        Pairs p = new Pairs();
        long[] st = new long[5];
        double[] mg = new double[1];
        int cap = 1 << 20;
        while (true) {
            p.i = new int[cap]; p.j = new int[cap]; p.sim = new double[cap];
            long count = nSimilarPairs(h, metric, n, dim, xFlat, minWeight, threshold, stripeRows, candidateCapacity, p.i, p.j, p.sim, st, mg);
            if (count > Integer.MAX_VALUE - 8) throw new IllegalStateException("more pairs than a Java array holds: " + count);
            if (count > cap) { cap = (int) count; continue; }
            p.i = Arrays.copyOf(p.i, (int) count); p.j = Arrays.copyOf(p.j, (int) count); p.sim = Arrays.copyOf(p.sim, (int) count);
            break;
        }
        p.pairsScreened = st[0]; p.candidates = st[1]; p.emitted = st[2]; p.stripes = (int) st[3]; p.regrown = (int) st[4]; p.margin = mg[0];
        return p;
    }

    /** (double) Math.round(similarity * 1000) / 1000, SciTopicFlow.java:1152,1467,1488 */
    public static double round3(double sim) { return (double) Math.round(sim * 1000) / 1000; }

    public static TopicLists docTopicsTop(NativeSampler s, double[] viewWeights, long d0, long d1, double threshold, int max) {
        long h = handleOf(s);
        TopicLists t = new TopicLists();
        t.rowOff = new long[(int) (d1 - d0 + 1)];
        long count = nDocTopicsTop(h, viewWeights, d0, d1, threshold, max, t.rowOff, null, null);
        if (count > Integer.MAX_VALUE - 8) throw new IllegalStateException("more entries than a Java array holds: " + count);
        t.topics = new int[(int) count];
        t.weights = new double[(int) count];
        if (count > 0) nDocTopicsTop(h, viewWeights, d0, d1, threshold, max, t.rowOff, t.topics, t.weights);
        return t;
    }

    /** [nGroups * K]; memberOff [nGroups + 1], members: entity ids of this sampler. */
    public static double[] entityTopicDistributions(NativeSampler s, int numTopics, double[] viewWeights, double threshold, int max, int roundDigits, long[] memberOff, long[] members) {
        double[] out = new double[Math.multiplyExact(memberOff.length - 1, numTopics)];
        nEntityTopicDistributions(handleOf(s), viewWeights, threshold, max, roundDigits, memberOff, members, out);
        return out;
    }
}
