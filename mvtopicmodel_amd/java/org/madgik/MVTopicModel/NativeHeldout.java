package org.madgik.MVTopicModel;

import java.lang.reflect.Field;

/**
 * Held-out evaluation on the GPU: the left-to-right document likelihood, the call that replaces
 * getMALLETProbEstimator().evaluateLeftToRight(testing, particles, resample, null) (FastQMVWVParallelTopicModel.java:3470-3478).
 * Contract: include/mvhdp.h (mvhdp_heldout_left_to_right) -- the estimator's mathematics with this library's random streams and summation
 * order, not MALLET's bytes.  The native lives in mvhdp_heldout_jni.cpp, built into the same libmvhdp_jni.so as NativeSampler's.
 */
public final class NativeHeldout {
    static {
        System.loadLibrary("mvhdp_jni");
    }

    private NativeHeldout() {}

    private static native double nLeftToRight(long handle, int m, int particles, int resample, long seed, long docBase, double[] alpha, double alphaSum, long[] docOff, int[] tokens, double[] docLl, double[] positionSum, long[] docTokens, long[] statsOut);

    /** What one evaluation returns: the total, and per document its log-likelihood and its in-vocabulary tokens. */
    public static final class Result {
        public double logLikelihood;
        public double[] docLogLikelihood;
        public double[] positionSum;          // S[n]: the particles' p(w_n | w_<n) added up, 0 at an out-of-vocabulary position; null unless asked for
        public long[] docTokens;
        public long tokens, oov, visits;

        public double perplexity() { return Math.exp(-logLikelihood / tokens); }
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

    /**
     * docOff[d] .. docOff[d + 1] index tokens (type ids of view 0; an id at or beyond the vocabulary is skipped).  particles = 10 and
     * resample = true are the arguments of MALLET's evaluator command line.
     */
    public static Result leftToRight(NativeSampler s, long[] docOff, int[] tokens, int particles, boolean resample, long seed, boolean wantPositionSums) {
        return leftToRight(s, 0, docOff, tokens, particles, resample, seed, 0L, null, 0.0, wantPositionSums);
    }

    /** view m; docBase: the global index of the first document (document shards); alpha (K values) with alphaSum replaces the model's. */
    public static Result leftToRight(NativeSampler s, int m, long[] docOff, int[] tokens, int particles, boolean resample, long seed, long docBase, double[] alpha, double alphaSum, boolean wantPositionSums) {
        long h = handleOf(s);
        if (docOff == null || docOff.length < 1) throw new IllegalArgumentException("docOff: at least one entry");
        if (tokens == null) throw new IllegalArgumentException("tokens: null");
        int d = docOff.length - 1;
        Result r = new Result();
        r.docLogLikelihood = new double[d];
        r.docTokens = new long[d];
        r.positionSum = wantPositionSums ? new double[tokens.length] : null;
        long[] st = new long[3];
        r.logLikelihood = nLeftToRight(h, m, particles, resample ? 1 : 0, seed, docBase, alpha, alphaSum, docOff, tokens, r.docLogLikelihood, r.positionSum, r.docTokens, st);
        r.tokens = st[0]; r.oov = st[1]; r.visits = st[2];
        return r;
    }
}
