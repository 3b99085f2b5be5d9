package org.madgik.MVTopicModel;

/**
 * JNI binding of libmvhdp.so (include/mvhdp.h): the MI355X replacement of the
 * FastQMVWVWorkerRunnable / FastQMVWVUpdaterRunnable threads that
 * FastQMVWVParallelTopicModel.estimate() submits every iteration.
 *
 * NOT compiled in the build image (no JDK there); kept as the reference-side
 * binding a maintainer adds.  See INTEGRATION.md for the patch to estimate().
 *
 * One instance = one model shard on one GPU.  Not thread-safe, like estimate().
 */
public final class NativeSampler implements AutoCloseable {

    static {
        System.loadLibrary("mvhdp_jni");   // libmvhdp_jni.so, linked against libmvhdp.so
    }

    public static final int SWEEP_REUSE_TREES = 0x1;
    public static final int SWEEP_NO_APPLY = 0x2;
    public static final int SWEEP_EXACT_CHAIN = 0x4;
    public static final int SWEEP_FROZEN = 0x10;       // the inferencer's call (nst = 1, nut = 0)
    public static final int SWEEP_LIVE = 0x20;         // the updater threads' own discipline: atomics on the shared counts
    public static final int SWEEP_SEGMENT_APPLY = 0x40; // deterministic: segments sampled one after the other, deltas applied in between
    public static final int SWEEP_ASYNC_EXCHANGE = 0x100;  // Group.sweep with SWEEP_LIVE: the all-reduce of sweep t beside sweep t+1 (then Group.drain())
    public static final int SWEEP_SEGMENT_OVERLAP = 0x80; // with SEGMENT_APPLY: the deltas of segment s are applied while segment s+1 samples (s+2 sees them)
    public static final int SWEEP_SHARD_BIRTHS = 0x200;  // Group.sweep with SWEEP_LIVE over a truncated HDP: every shard gives birth chunk by chunk, every replica activates what any reached
    public static int sweepLiveSegments(int n) { return (n & 0xff) << 16; }
    public static int sweepOnlySegment(int s) { return ((s + 1) & 0xff) << 24; }   // only segment s of the n segments

    /** What one sweep reports: the three branch counters of the worker plus bookkeeping. */
    public static final class SweepStats {
        public long tokens, changed, newMassCnt, topicDocMassCnt, wordFTreeMassCnt, oovSkipped, abortedDocs, exactFallbacks;
        public int activatedTopic, activatedModality;
        public long activationKey;
        public double sweepKernelMs, totalMs;
        public int activations;          // topics activated during the call (a segmented sweep: one per segment border; a live sweep in its live-rows form: chunk by chunk, any number)
    }

    private long handle;   // mvhdp_handle

    public NativeSampler(int numTopics, int[] numTypes, int device, long docIdBase) {
        handle = nCreate(numTopics, numTypes, device, docIdBase);
    }

    /** tokens = FeatureSequence indices of every entity's view m, docOff = CSR offsets (size by getLength()). */
    public void setCorpus(int m, long[] docOff, int[] tokens) { nSetCorpus(handle, m, docOff, tokens); }
    public void setAssignments(int m, int[] z) { nSetAssignments(handle, m, z); }
    public void getAssignments(int m, int[] z) { nGetAssignments(handle, m, z); }
    /** present[d] = data.get(d).Assignments[m] != null: an instance with an EMPTY FeatureSequence is not a missing view (lines 3348-3373, 2873-2886). */
    public void setViewPresence(int m, boolean[] present) { nSetViewPresence(handle, m, present); }

    public void setHyper(double[][] alpha, double[] alphaSum, double[] beta, double[] betaSum, double[] gamma,
                         double[][] p_a, double[][] p_b, boolean[] inactive) {
        nSetHyper(handle, alpha, alphaSum, beta, betaSum, gamma, p_a, p_b, inactive);
    }

    public void buildCounts() { nBuildCounts(handle); }
    public void buildTrees() { nBuildTrees(handle); }
    public void getCounts(int m, int[] typeTopicCountsFlat, int[] tokensPerTopic) { nGetCounts(handle, m, typeTopicCountsFlat, tokensPerTopic); }
    public void getDocTopicHist(int m, int[] histFlat, int histLen, int[] docLengthCounts) { nGetDocTopicHist(handle, m, histFlat, histLen, docLengthCounts); }
    public void getAlpha(double[] alphaFlat, boolean[] inactive) { nGetAlpha(handle, alphaFlat, inactive); }

    /** pOverride: [D*M*M] view weights drawn as WorkerRunnable lines 327-337, or null to draw them on the device. */
    public SweepStats sweep(int sweepIdx, long seed, int flags, double[] pOverride) {
        SweepStats st = new SweepStats();
        nSweep(handle, sweepIdx, seed, flags, pOverride, st);
        return st;
    }

    /** Multi-GPU: after the all-reduce of the delta buffer; (topic, modality) = winner of the MIN-reduced activation key. */
    public void applyDelta(int activatedTopic, int activatedModality) { nApplyDelta(handle, activatedTopic, activatedModality); }
    public double[] modelLogLikelihood(int numModalities) { double[] ll = new double[numModalities]; nModelLogLikelihood(handle, ll); return ll; }
    /** countHistogram of optimizeBeta (lines 2295-2309): hist[c] = (type, topic) pairs of view m holding count c. */
    public void getCountHistogram(int m, int[] hist) { nGetCountHistogram(handle, m, hist); }
    /** optimizeP (lines 2706-2792): sums[m*M+i] = sum over the entities, in entity order, of pDistr_Mean[m][i][doc]. */
    public double[] viewOverlapSums(int numModalities) { double[] s = new double[numModalities * numModalities]; nViewOverlapSums(handle, s); return s; }
    /** optimizeGamma's document level (lines 2415-2433): {qs, qw}, every entity drawing from its own counter-based stream. */
    public double[] gammaDocStatistics(int m, double gammaM, long seed, int round) { double[] o = new double[2]; nGammaDocStatistics(handle, m, gammaM, seed, round, o); return o; }
    /** optimizeDP's view-table simulation PTM:2454-2488 over topicDocCounts[m] (hist [K][histLen], of the whole model): mk [K] and active [K] are filled. */
    public void dpTableStatistics(int m, int[] hist, int histLen, double[] conc, long seed, int round, double[] mk, byte[] active) { nDpTableStatistics(handle, m, hist, histLen, conc, seed, round, mk, active); }

    /**
     * n sweeps (indices firstIdx .. firstIdx+n-1) enqueued back to back, one synchronisation at the end: the iteration loop
     * of estimate() (lines 1146-1239) without a host round trip per iteration.  Same integers as n calls of sweep().
     */
    public SweepStats[] sweepMany(int firstIdx, int n, long seed, int flags) {
        long[] flat = new long[n * 8];
        nSweepMany(handle, firstIdx, n, seed, flags, flat);
        SweepStats[] out = new SweepStats[n];
        for (int i = 0; i < n; i++) out[i] = statsFromFlat(flat, i);
        return out;
    }

    static SweepStats statsFromFlat(long[] flat, int i) {
        SweepStats st = new SweepStats();
        st.tokens = flat[8 * i]; st.changed = flat[8 * i + 1]; st.newMassCnt = flat[8 * i + 2]; st.topicDocMassCnt = flat[8 * i + 3];
        st.wordFTreeMassCnt = flat[8 * i + 4]; st.oovSkipped = flat[8 * i + 5]; st.abortedDocs = flat[8 * i + 6]; st.exactFallbacks = flat[8 * i + 7];
        return st;
    }

    /** mvhdp_emb_config: the shape of TopicWordEmbeddings(alphabet[0], numColumns, numContextColumns, window, numTopics, ..) (TWE:126-163)
     *  and what countWords / train take; the defaults are the reference's (PTM:523, FLOW:74, train(data, threads, 5, 2)). */
    public static final class EmbConfig {
        public int numColumns = 200, numContextColumns = 50, window = 5, numSamples = 5, minDocLength = 10, sigmoidCacheSize = 1000;
        public boolean withTopics = true;                     // false: WordEmbeddings (FLOW:115-136; no topic rows, no context columns)
        public long samplingTableSize = 100000000L;
        public double samplingFactor = 1e-4, minExp = -6.0, maxExp = 6.0;
    }
    /** What one embTrain reports (mvhdp_emb_stats), summed over its epochs. */
    public static final class EmbStats {
        public long wordsSoFar, wordsSampled, wordsConsidered, docsSkipped, calls, negativesSkipped, lastEpochCalls;
        public double residual, lastEpochResidual, kernelMs;
        public double meanError() { return lastEpochCalls == 0 ? 0.0 : lastEpochResidual / lastEpochCalls; }   // getMeanError TWER:70-79
    }
    public static final int EMB_SERIAL = 0x1;             // one wave, entities in id order (deterministic); default: Hogwild
    /** new TopicWordEmbeddings TWE:126-163 on the device; weightsFlat [R*C] (R = V_0, + K with topics) or null: drawn on the device. */
    public void embInit(EmbConfig c, double[] weightsFlat, long seed) {
        int[] ints = {c.numColumns, c.numContextColumns, c.withTopics ? 1 : 0, c.window, c.numSamples, c.minDocLength, c.sigmoidCacheSize};
        nEmbInit(handle, ints, c.samplingTableSize, new double[] {c.samplingFactor, c.minExp, c.maxExp}, weightsFlat, seed);
    }
    /** matrix.countWords(data, samplingFactor) TWE:341-401 over the view-0 tokens set with setCorpus (cumulative, as the reference's). */
    public void embCountWords() { nEmbCountWords(handle); }
    /** matrix.train(data, numThreads, numSamples, epochs) TWE:423-483 over view 0 and its current assignments. */
    public EmbStats embTrain(int epochs, long seed, int round, int flags) {
        long[] l = new long[7]; double[] d = new double[3];
        nEmbTrain(handle, epochs, seed, round, flags, l, d);
        EmbStats st = new EmbStats();
        st.wordsSoFar = l[0]; st.wordsSampled = l[1]; st.wordsConsidered = l[2]; st.docsSkipped = l[3]; st.calls = l[4];
        st.negativesSkipped = l[5]; st.lastEpochCalls = l[6]; st.residual = d[0]; st.lastEpochResidual = d[1]; st.kernelMs = d[2];
        return st;
    }
    /** weights / negativeWeights [R*C] row-major, or null: getWordVectors (rows 0..V_0) / getTopicVectors (rows V_0..) TWE:726-745. */
    public void embGetVectors(double[] weightsFlat, double[] negativeWeightsFlat) { nEmbGetVectors(handle, weightsFlat, negativeWeightsFlat); }
    public void embSetVectors(double[] weightsFlat, double[] negativeWeightsFlat) { nEmbSetVectors(handle, weightsFlat, negativeWeightsFlat); }
    /** wordCounts [V_0] and retentionProbability [V_0] (or null); returns totalWords. */
    public long embWordStats(long[] counts, double[] retention) { long[] t = new long[1]; nEmbWordStats(handle, counts, retention, t); return t[0]; }
    public void embSamplingTable(long first, int[] types) { nEmbSamplingTable(handle, first, types); }
    /** CalcSoftmaxTopicWordProbabilities PTM:337-367: expDotProductValues [K*V_0] (or null), sumExpValues [K] accumulated over calls. */
    public void embSoftmax(boolean resetSums, double[] expDotFlat, double[] sumExp) { nEmbSoftmax(handle, resetSums, expDotFlat, sumExp); }
    /** findClosest TWE:485-540: the n (1..64) closest words and topics by cosine, IDSorter order. */
    public void embNearest(double[] query, int n, int[] words, double[] wordSims, int[] topics, double[] topicSims) { nEmbNearest(handle, query, n, words, wordSims, topics, topicSims); }
    public void embRelease() { nEmbRelease(handle); }
    /**
     * useVectorsLambda (WRK:504-507, PTM:2673-2678): lambda = 0 switches the mix off, 0 &lt; lambda &lt;= 1 on.  expDotFlat [K*V_0] / sumExp [K] are
     * expDotProductValues / sumExpValues; both null: the table the last embSoftmax left on the device.  Invalidates the F+trees.
     */
    public void setVectorsMix(double lambda, double[] expDotFlat, double[] sumExp) { nSetVectorsMix(handle, lambda, expDotFlat, sumExp); }
    /** lambda (0: off); mixFlat [V_0*K] or null receives lambda * (e / S) as the device holds it. */
    public double getVectorsMix(double[] mixFlat) { return nGetVectorsMix(handle, mixFlat); }

    /**
     * The sweep's own choices (mvhdp_tuning): none of them changes a result.  learntWalkStep / treeBranchShare are what the
     * library's walk-threshold search has found -- read them from one sampler and hand them to another (a document shard, a
     * resumed chain) and it does not search again.
     */
    /** getSortedWords(m) PTM:1792-1811 cut at n (1..64): typesFlat / counts [K*n] (unfilled slots -1 / 0), nonzero [K] = sortedWords.size(). */
    public void topWords(int m, int n, int[] typesFlat, int[] counts, int[] nonzero) { nTopWords(handle, m, n, typesFlat, counts, nonzero); }
    /** calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230: discrWeightPerModality [M]; typeWeight [V_m] = typeDiscrWeight[m], or null. */
    public double[] discrWeights(int numModalities, int m, double[] typeWeight) { double[] w = new double[numModalities]; nDiscrWeights(handle, w, m, typeWeight); return w; }

    /** What FastQMVWVTopicModelDiagnostics(model, numTopWords) computes (DIAG:53-236): scores [13*K] in the row order of DIAG:104-116
     *  (TopicScores.scores), wordScores [13*K*N] (topicWordScores), the co-document matrices [K*N*N], the view-0 top words and the
     *  accumulators of collectDocumentStatistics, discrWeightPerModality. */
    public static final class Diagnostics {
        public static final String[] ROWS = {"tokens", "document_entropy", "word-length", "coherence", "normDiscrWeight", "discrWeight", "uniform_dist",
                                             "corpus_dist", "eff_num_words", "token-doc-diff", "rank_1_docs", "allocation_ratio", "allocation_count"};
        public final int numTopics, numTopWords;
        public final double[] scores, wordScores, sumCountLogCount, discrWeightPerModality;
        public final int[] codoc, topTypes, topCounts, nonzero, numRank1Documents, numNonZeroDocuments, numDocumentsAtProportions, wordTypeCounts;
        public final long[] numTokens = new long[1];
        Diagnostics(int K, int N, int V0, int M) {
            numTopics = K; numTopWords = N;
            scores = new double[ROWS.length * K]; wordScores = new double[ROWS.length * K * N]; sumCountLogCount = new double[K];
            discrWeightPerModality = new double[M]; codoc = new int[K * N * N]; topTypes = new int[K * N]; topCounts = new int[K * N];
            nonzero = new int[K]; numRank1Documents = new int[K]; numNonZeroDocuments = new int[K]; numDocumentsAtProportions = new int[K * 7];
            wordTypeCounts = new int[V0];
        }
        public double score(int row, int topic) { return scores[row * numTopics + topic]; }
    }
    /** wordLength: String.length() of every view-0 type (alphabet[0]), or null (the word-length row is then NaN). */
    public Diagnostics diagnostics(int numTopics, int numTypes0, int numModalities, int numTopWords, int[] wordLength) {
        Diagnostics d = new Diagnostics(numTopics, numTopWords, numTypes0, numModalities);
        nDiagnostics(handle, numTopWords, wordLength, d.scores, d.wordScores, d.codoc, d.topTypes, d.topCounts, d.nonzero, d.numRank1Documents,
                     d.numNonZeroDocuments, d.numDocumentsAtProportions, d.sumCountLogCount, d.wordTypeCounts, d.numTokens, d.discrWeightPerModality);
        return d;
    }

    public static final class Tuning {
        public int forcePrimary, narrow = -1, walkFixed, singleStream, live16 = -1;
        public int[] learntWalkStep = {-1, -1, -1};
        public double primaryMinShare;
        public double[] walkTheta = new double[8], treeBranchShare = new double[8];
    }

    public Tuning getTuning() {
        int[] iv = new int[8]; double[] dv = new double[17];
        nGetTuning(handle, iv, dv);
        Tuning t = new Tuning();
        t.forcePrimary = iv[0]; t.narrow = iv[1]; t.walkFixed = iv[2]; t.singleStream = iv[3]; t.live16 = iv[4];
        t.learntWalkStep = new int[] {iv[5], iv[6], iv[7]};
        t.primaryMinShare = dv[0];
        System.arraycopy(dv, 1, t.walkTheta, 0, 8); System.arraycopy(dv, 9, t.treeBranchShare, 0, 8);
        return t;
    }

    public void setTuning(Tuning t) {
        int[] iv = {t.forcePrimary, t.narrow, t.walkFixed, t.singleStream, t.live16, t.learntWalkStep[0], t.learntWalkStep[1], t.learntWalkStep[2]};
        double[] dv = new double[17];
        dv[0] = t.primaryMinShare;
        System.arraycopy(t.walkTheta, 0, dv, 1, 8); System.arraycopy(t.treeBranchShare, 0, dv, 9, 8);
        nSetTuning(handle, iv, dv);
    }

    /**
     * Document shards on several GPUs with the exchange step inside the library (mvhdp_group_*): what the queue mesh between
     * sampler and updater threads and the CyclicBarrier do inside the reference's one JVM (lines 1042-1049, 1232).  Every member
     * holds a contiguous range of entities (docIdBase = global index of its first entity) and a full replica of the model.
     */
    public static final class Group implements AutoCloseable {
        private long g;
        private final int members;

        /** One JVM drives all its GPUs: one NativeSampler per device. */
        public Group(NativeSampler[] samplers) {
            long[] hs = new long[samplers.length];
            for (int i = 0; i < hs.length; i++) hs[i] = samplers[i].handle;
            g = nGroupCreate(hs);
            members = hs.length;
        }

        private Group(long g) { this.g = g; this.members = 1; }

        /** One JVM per GPU: rank 0 calls uniqueId(), the launcher hands the 128 bytes to every rank, every rank calls this. */
        public static Group ofRank(NativeSampler sampler, byte[] id, int rank, int nranks) {
            return new Group(nGroupCreateRank(sampler.handle, id, rank, nranks));
        }

        public static byte[] uniqueId() { byte[] id = new byte[128]; nGroupUniqueId(id); return id; }

        /** buildInitialTypeTopicCounts (lines 600-652) over all shards. */
        public void buildCounts() { nGroupBuildCounts(g); }

        /** One sweep of the whole model; flags: SWEEP_LIVE / SWEEP_SEGMENT_APPLY (+ sweepLiveSegments), SWEEP_EXACT_CHAIN.  A host that shards
         *  a truncated HDP passes SWEEP_LIVE | SWEEP_SHARD_BIRTHS: topics are born on every shard chunk by chunk (UPD:263-270, WRK:522-526) and the
         *  exchange carries a table of K birth keys instead of one, so a step activates any number of topics (stats: activations, the lowest-index
         *  newborn in activatedTopic).  Every rank passes the same flags. */
        public SweepStats[] sweep(int sweepIdx, long seed, int flags) {
            long[] flat = new long[members * 8];
            int[] act = new int[3];
            double exchangeMs = nGroupSweep(g, sweepIdx, seed, flags, flat, act);
            SweepStats[] out = new SweepStats[members];
            for (int i = 0; i < members; i++) {
                out[i] = statsFromFlat(flat, i);
                out[i].activatedTopic = act[0]; out[i].activatedModality = act[1]; out[i].activations = act[2];
                out[i].totalMs = exchangeMs;
            }
            return out;
        }

        /** After SWEEP_ASYNC_EXCHANGE sweeps: lands what is on the wire, every replica is the global model again. */
        public void drain() { nGroupDrain(g); }

        /** This rank cannot go on: its next sweep contributes nothing and fails on EVERY rank together (nobody waits in a collective). */
        public void abort() { nGroupAbort(g); }

        // The steps either side of the sweep for the sharded model (what estimate() does every optimizeInterval and every tenth
        // iteration, lines 1173-1210 and 1296-1320): statistics of the replicated counts are any member's, statistics over the
        // entities are put together from the members in entity order.  setHyper: call NativeSampler.setHyper on every member.
        public double[] modelLogLikelihood(int numModalities) { double[] ll = new double[numModalities]; nGroupModelLogLikelihood(g, ll); return ll; }
        public void getDocTopicHist(int m, int[] histFlat, int histLen, int[] docLengthCounts) { nGroupGetDocTopicHist(g, m, histFlat, histLen, docLengthCounts); }
        public void getCountHistogram(int m, int[] hist) { nGroupGetCountHistogram(g, m, hist); }
        public double[] viewOverlapSums(int numModalities) { double[] s = new double[numModalities * numModalities]; nGroupViewOverlapSums(g, s); return s; }
        public double[] gammaDocStatistics(int m, double gammaM, long seed, int round) { double[] o = new double[2]; nGroupGammaDocStatistics(g, m, gammaM, seed, round, o); return o; }
        /** the diagnostics of the whole sharded model; top words and discrimination weights are any member's (topWords / discrWeights there) */
        public Diagnostics diagnostics(int numTopics, int numTypes0, int numModalities, int numTopWords, int[] wordLength) {
            Diagnostics d = new Diagnostics(numTopics, numTopWords, numTypes0, numModalities);
            nGroupDiagnostics(g, numTopWords, wordLength, d.scores, d.wordScores, d.codoc, d.topTypes, d.topCounts, d.nonzero, d.numRank1Documents,
                              d.numNonZeroDocuments, d.numDocumentsAtProportions, d.sumCountLogCount, d.wordTypeCounts, d.numTokens, d.discrWeightPerModality);
            return d;
        }

        @Override
        public void close() { if (g != 0) { nGroupDestroy(g); g = 0; } }
    }

    /**
     * Safe from a finalizer or a shutdown hook (after the HIP runtime has gone the library frees host memory only) and when it
     * races a second close: the native side drops the handle from its registry under a lock and ignores a handle it does not know.
     */
    @Override
    public synchronized void close() {
        if (handle != 0) { long h = handle; handle = 0; nDestroy(h); }
    }

    private static native long nCreate(int numTopics, int[] numTypes, int device, long docIdBase);
    private static native void nDestroy(long h);
    private static native void nSetCorpus(long h, int m, long[] docOff, int[] tokens);
    private static native void nSetAssignments(long h, int m, int[] z);
    private static native void nGetAssignments(long h, int m, int[] z);
    private static native void nSetViewPresence(long h, int m, boolean[] present);
    private static native void nSetHyper(long h, double[][] alpha, double[] alphaSum, double[] beta, double[] betaSum,
                                         double[] gamma, double[][] p_a, double[][] p_b, boolean[] inactive);
    private static native void nBuildCounts(long h);
    private static native void nBuildTrees(long h);
    private static native void nGetCounts(long h, int m, int[] typeTopicCountsFlat, int[] tokensPerTopic);
    private static native void nGetDocTopicHist(long h, int m, int[] histFlat, int histLen, int[] docLengthCounts);
    private static native void nGetAlpha(long h, double[] alphaFlat, boolean[] inactive);
    private static native void nSweep(long h, int sweepIdx, long seed, int flags, double[] pOverride, SweepStats out);
    private static native void nApplyDelta(long h, int topic, int modality);
    private static native void nModelLogLikelihood(long h, double[] out);
    private static native void nSweepMany(long h, int firstIdx, int n, long seed, int flags, long[] statsFlat);
    private static native void nGetTuning(long h, int[] ints, double[] doubles);
    private static native void nSetTuning(long h, int[] ints, double[] doubles);
    private static native long nGroupCreate(long[] handles);
    private static native void nGroupUniqueId(byte[] id);
    private static native long nGroupCreateRank(long h, byte[] id, int rank, int nranks);
    private static native void nGroupDestroy(long g);
    private static native void nGroupBuildCounts(long g);
    private static native double nGroupSweep(long g, int sweepIdx, long seed, int flags, long[] statsFlat, int[] act);
    private static native void nGetCountHistogram(long h, int m, int[] hist);
    private static native void nViewOverlapSums(long h, double[] sums);
    private static native void nGammaDocStatistics(long h, int m, double gammaM, long seed, int round, double[] out);
    private static native void nDpTableStatistics(long h, int m, int[] hist, int histLen, double[] conc, long seed, int round, double[] mk, byte[] active);
    private static native void nGroupAbort(long g);
    private static native void nGroupDrain(long g);
    private static native void nGroupModelLogLikelihood(long g, double[] out);
    private static native void nGroupGetDocTopicHist(long g, int m, int[] histFlat, int histLen, int[] docLengthCounts);
    private static native void nGroupGetCountHistogram(long g, int m, int[] hist);
    private static native void nGroupViewOverlapSums(long g, double[] sums);
    private static native void nGroupGammaDocStatistics(long g, int m, double gammaM, long seed, int round, double[] out);
    private static native void nTopWords(long h, int m, int n, int[] typesFlat, int[] counts, int[] nonzero);
    private static native void nDiscrWeights(long h, double[] perView, int m, double[] typeWeight);
    private static native void nDiagnostics(long h, int n, int[] wordLength, double[] scores, double[] wordScores, int[] codoc, int[] topTypes,
                                            int[] topCounts, int[] nonzero, int[] rank1Docs, int[] nonzeroDocs, int[] atProportions,
                                            double[] sumCountLogCount, int[] wordTypeCounts, long[] numTokens, double[] perView);
    private static native void nGroupDiagnostics(long g, int n, int[] wordLength, double[] scores, double[] wordScores, int[] codoc, int[] topTypes,
                                                 int[] topCounts, int[] nonzero, int[] rank1Docs, int[] nonzeroDocs, int[] atProportions,
                                                 double[] sumCountLogCount, int[] wordTypeCounts, long[] numTokens, double[] perView);
    private static native void nEmbInit(long h, int[] ints, long tableSize, double[] doubles, double[] weights, long seed);
    private static native void nEmbCountWords(long h);
    private static native void nEmbTrain(long h, int epochs, long seed, int round, int flags, long[] longs, double[] doubles);
    private static native void nEmbGetVectors(long h, double[] weights, double[] negativeWeights);
    private static native void nEmbSetVectors(long h, double[] weights, double[] negativeWeights);
    private static native void nEmbWordStats(long h, long[] counts, double[] retention, long[] totalWords);
    private static native void nEmbSamplingTable(long h, long first, int[] types);
    private static native void nEmbSoftmax(long h, boolean resetSums, double[] expDot, double[] sumExp);
    private static native void nEmbNearest(long h, double[] query, int n, int[] words, double[] wordSims, int[] topics, double[] topicSims);
    private static native void nEmbRelease(long h);
    private static native void nSetVectorsMix(long h, double lambda, double[] expDot, double[] sumExp);
    private static native double nGetVectorsMix(long h, double[] mix);
}
