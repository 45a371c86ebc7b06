// h_comm.inc -- part of krisp_hip.hip (one translation unit): host: the ONE exchange step of the
// multi-GPU flow, inside the library -- one process per GPU, genomes sharded over the ranks, sort
// and local intersect without any collective, then a binary-tree reduction of the candidate lists
// (the reference reduces the same way, as a tree of pairwise file merges on one host:
// krisp_fasta/intersectAmplicons.py:256-307), a broadcast of the survivors and a gather of the
// records.  Transport: RCCL point-to-point / collectives on the context's stream, straight from
// and into device buffers (xGMI between the GPUs of a node; the lists are the few thousand
// candidates the monotone filter leaves, SURVEY 8e).  A second transport moves the same bytes
// through files in a directory: the rehearsal form (ranks sharing one GPU, where RCCL refuses
// duplicate devices) that lets the tree logic and the device merges run under test on a one-GPU box.
// ----------------------------------------------------------------------------
// The communicator's watchdog (round 6, VERDICT r5 item 5a).  ncclSend / ncclRecv / the collectives have no timeout, and a
// rank that died, or never arrived, leaves its partners inside a call or behind a stream synchronisation for good.  One host
// thread per RCCL communicator: while an exchange call of this library is in progress (WatchScope arms it at entry, with the
// deadline KRISP_COMM_TIMEOUT seconds -- default 600, kr_comm_set_timeout -- and disarms it at exit) it polls
// ncclCommGetAsyncError five times a second; on an asynchronous error or when the deadline passes it says so on stderr and calls
// ncclCommAbort from its own thread -- the documented way to unblock the calls and kernels of a communicator --, the call in
// progress then fails with an error code (the command line exits non-zero with it: no rank waits for a dead one, nothing is
// re-executed).  If the blocked call does not come back within a grace period after the abort (or the communicator does not
// exist yet: ncclCommInitRank waiting for a rank that never joins) the thread ends the process with status 124.
static int comm_timeout_default() {
    const char* e = getenv("KRISP_COMM_TIMEOUT");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 600;
}

struct CommWatch {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool stop = false;
    int depth = 0;                  // exchange calls in progress (nested: kr_cands_reduce -> kr_comm_allreduce): armed while > 0
    std::chrono::steady_clock::time_point deadline;
    const char* what = "";
    std::atomic<int> fired{0};      // 1 = deadline, 2 = asynchronous error: the communicator was aborted
    int grace_s = 10;
};

struct kr_comm {
    int rank = 0, world = 1;
    bool rccl = false;
    ncclComm_t nccl = nullptr;
    CommWatch* watch = nullptr;
    std::string dir;              // file transport
    std::map<int, u64> sent, rcvd;   // file transport: messages so far to / from each peer (both ends of a
                                     // directed pair count alike, so the number names the message)
    DevBuf scratch;               // device u64[16]: counts and small reductions
    DevBuf gather;                // kr_comm_allgather: own bytes, then every rank's
    int timeout_s = comm_timeout_default();     // the file transport's wait for a message; the watchdog's deadline per exchange call
    // the candidate exchange: a list travels as ONE message of agreed size -- ex_cap entries, then this header --
    // (members, not locals: the stream reads / writes them after the call that queued the copy has gone on)
    u64 hdr_out[2] = {0, 0}, hdr_in[2] = {0, 0};      // {entries that count, poison}
    // what the exchange cost (kr_debug_comm): host synchronisations, point-to-point calls, collectives, microseconds
    // inside kr_cands_reduce / kr_cands_bcast
    int64_t n_sync = 0, n_p2p = 0, n_coll = 0, n_reduce = 0;
    double ex_us = 0;
};
static void watch_main(kr_comm* m) {
    CommWatch* w = m->watch;
    std::unique_lock<std::mutex> lk(w->mu);
    for (;;) {
        w->cv.wait_for(lk, std::chrono::milliseconds(200));
        if (w->stop) return;
        if (w->depth <= 0) continue;
        const bool late = std::chrono::steady_clock::now() > w->deadline;
        ncclComm_t h = m->nccl;
        ncclResult_t ae = ncclSuccess;
        const bool bad = h && ncclCommGetAsyncError(h, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress;
        if (!late && !bad) continue;
        w->fired = late ? 1 : 2;
        fprintf(stderr, "[krisp_hip] rank %d of %d: %s: %s -- aborting the communicator\n", m->rank, m->world, w->what,
                late ? "no answer from the other ranks within the exchange deadline (KRISP_COMM_TIMEOUT)"
                     : ncclGetErrorString(ae));
        if (h) {
            lk.unlock();
            (void)ncclCommAbort(h);             // (from this thread: the blocked call and its kernels give up)
            lk.lock();
            const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(w->grace_s);
            while (w->depth > 0 && !w->stop && std::chrono::steady_clock::now() < until)
                w->cv.wait_for(lk, std::chrono::milliseconds(100));
            if (w->depth <= 0 || w->stop) return;      // the call came back with its error: the caller takes it from here
        }
        fprintf(stderr, "[krisp_hip] rank %d of %d: %s did not return: ending this process (status 124)\n", m->rank, m->world,
                w->what);
        fflush(stderr);
        _exit(124);
    }
}

static void watch_start(kr_comm* m) {
    m->watch = new CommWatch();
    try {
        m->watch->th = std::thread(watch_main, m);
    } catch (...) {         // (no thread to be had: the exchange runs without its watchdog, as before round 6)
        delete m->watch;
        m->watch = nullptr;
    }
}

static void watch_stop(kr_comm* m) {
    if (!m->watch) return;
    {
        std::lock_guard<std::mutex> lk(m->watch->mu);
        m->watch->stop = true;
    }
    m->watch->cv.notify_all();
    if (m->watch->th.joinable()) m->watch->th.join();
    delete m->watch;
    m->watch = nullptr;
}

// an exchange call in progress: the watchdog's deadline runs from here (nested scopes keep the outermost one's)
struct WatchScope {
    CommWatch* w;
    WatchScope(kr_ctx* c, const char* what) : w(c && c->comm ? c->comm->watch : nullptr) {
        if (!w) return;
        std::lock_guard<std::mutex> lk(w->mu);
        if (w->depth++ == 0) {
            w->what = what;
            w->deadline = std::chrono::steady_clock::now() + std::chrono::seconds(c->comm->timeout_s);
        }
    }
    ~WatchScope() {
        if (!w) return;
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->depth--;
        }
        w->cv.notify_all();
    }
};
static bool comm_dead(const kr_ctx* c) { return c->comm && c->comm->watch && c->comm->watch->fired.load() != 0; }
#define COMM_ALIVE(c, who)                                                                                              \
    do {                                                                                                                \
        if (comm_dead(c)) return fail((c), KR_ERR_STATE, "%s: the communicator was aborted by its watchdog (a rank failed or did not answer)", who); \
    } while (0)

static int comm_sync(kr_ctx* c) {       // a host synchronisation inside the exchange (counted)
    if (c->comm) c->comm->n_sync++;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    COMM_ALIVE(c, "exchange");          // (an aborted communicator's kernels end, the stream drains: the data is void)
    return KR_OK;
}

#define NCCLCHK(c, call)                                                                                   \
    do {                                                                                                   \
        ncclResult_t _r = (call);                                                                          \
        if (_r != ncclSuccess)                                                                             \
            return fail((c), KR_ERR_HIP, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(_r), __FILE__, \
                        __LINE__);                                                                         \
    } while (0)

int kr_comm_unique_id(uint8_t* id) {
    if (!id) return KR_ERR_PARAM;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) {
        g_last_error = "ncclGetUniqueId failed";
        return KR_ERR_HIP;
    }
    static_assert(sizeof(u) == KR_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(id, &u, sizeof u);
    return KR_OK;
}

static int comm_common(kr_ctx* c, int rank, int world) {
    if (!c) return KR_ERR_PARAM;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, KR_ERR_PARAM, "rank %d of %d", rank, world);
    if (c->comm) return fail(c, KR_ERR_STATE, "this context already has a communicator");
    HIPCHK(c, hipSetDevice(c->device));
    c->comm = new kr_comm();
    c->comm->rank = rank;
    c->comm->world = world;
    int rc = ensure(c, c->comm->scratch, 16 * 8);
    if (rc) { delete c->comm; c->comm = nullptr; }
    return rc;
}

int kr_comm_init(kr_ctx* c, int rank, int world, const uint8_t* id) {
    if (!id) return KR_ERR_PARAM;
    int rc = comm_common(c, rank, world);
    if (rc) return rc;
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    watch_start(c->comm);
    ncclResult_t r;
    {
        WatchScope ws(c, "ncclCommInitRank (waiting for every rank to join)");
        r = ncclCommInitRank(&c->comm->nccl, world, u, rank);
    }
    if (r != ncclSuccess) {
        watch_stop(c->comm);
        release(c, c->comm->scratch);
        delete c->comm;
        c->comm = nullptr;
        return fail(c, KR_ERR_HIP, "ncclCommInitRank(rank %d of %d) failed: %s", rank, world, ncclGetErrorString(r));
    }
    c->comm->rccl = true;
    return KR_OK;
}

int kr_comm_init_dir(kr_ctx* c, int rank, int world, const char* dir) {
    if (!dir || !*dir) return KR_ERR_PARAM;
    int rc = comm_common(c, rank, world);
    if (rc) return rc;
    c->comm->dir = dir;
    c->shared_gpu = true;          // (ranks that rehearse on one GPU share its memory: no placement search, h_core.inc)
    (void)mkdir(dir, 0700);
    return KR_OK;
}

int kr_comm_destroy(kr_ctx* c) {
    if (!c || !c->comm) return KR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const bool aborted = comm_dead(c);
    watch_stop(c->comm);
    if (c->comm->rccl && c->comm->nccl && !aborted) (void)ncclCommDestroy(c->comm->nccl);     // (ncclCommAbort has freed an aborted one)
    if (!c->comm->dir.empty()) {
        // file transport: the last rank to leave finds the run's message directory empty and removes it, and the
        // directory above it once no other run has one there (rmdir of a non-empty directory fails: nothing is lost)
        (void)rmdir(c->comm->dir.c_str());
        const size_t cut = c->comm->dir.find_last_of('/');
        if (cut != std::string::npos && cut > 2 && c->comm->dir.compare(cut - 2, 2, ".d") == 0)     // (distributed.connect's <name>.d only)
            (void)rmdir(c->comm->dir.substr(0, cut).c_str());
    }
    release(c, c->comm->scratch);
    release(c, c->comm->gather);
    delete c->comm;
    c->comm = nullptr;
    return KR_OK;
}

int kr_comm_rank(kr_ctx* c) { return c && c->comm ? c->comm->rank : 0; }
int kr_comm_world(kr_ctx* c) { return c && c->comm ? c->comm->world : 1; }
int kr_comm_rccl_ranks(kr_ctx* c) {
    if (!c || !c->comm || !c->comm->rccl || !c->comm->nccl) return 0;
    int n = 0;
    return ncclCommCount(c->comm->nccl, &n) == ncclSuccess ? n : 0;
}

int kr_comm_set_timeout(kr_ctx* c, int seconds) {
    if (!c || !c->comm) return fail(c, KR_ERR_STATE, "kr_comm_set_timeout: no communicator");
    if (seconds < 1) return fail(c, KR_ERR_PARAM, "kr_comm_set_timeout: seconds >= 1");
    c->comm->timeout_s = seconds;
    return KR_OK;
}

// ---- file transport: message number `seq` from src to dst = <dir>/m<seq>_<src>_<dst> (written
// under a temporary name, then renamed: a reader never sees a partial file)
static std::string msg_path(const kr_comm* m, u64 seq, int src, int dst) {
    char b[96];
    snprintf(b, sizeof b, "/m%llu_%d_%d", (unsigned long long)seq, src, dst);
    return m->dir + b;
}
static int file_put(kr_ctx* c, const void* host, size_t bytes, int dst) {
    kr_comm* m = c->comm;
    const std::string path = msg_path(m, m->sent[dst]++, m->rank, dst), tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(c, KR_ERR_HIP, "cannot write %s", tmp.c_str());
    const size_t w = bytes ? fwrite(host, 1, bytes, f) : 0;
    fclose(f);
    if (w != bytes || rename(tmp.c_str(), path.c_str()) != 0) return fail(c, KR_ERR_HIP, "cannot write %s", path.c_str());
    return KR_OK;
}
static int file_get(kr_ctx* c, void* host, size_t bytes, int src) {
    kr_comm* m = c->comm;
    const std::string path = msg_path(m, m->rcvd[src]++, src, m->rank);
    const auto t0 = std::chrono::steady_clock::now();
    FILE* f = nullptr;
    while (!(f = fopen(path.c_str(), "rb"))) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(m->timeout_s))
            return fail(c, KR_ERR_HIP, "rank %d: no message %s within %d s", m->rank, path.c_str(), m->timeout_s);
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    const size_t r = bytes ? fread(host, 1, bytes, f) : 0;
    fclose(f);
    (void)unlink(path.c_str());
    if (r != bytes) return fail(c, KR_ERR_HIP, "message %s: %zu of %zu bytes", path.c_str(), r, bytes);
    return KR_OK;
}

// ---- point-to-point on DEVICE buffers
static int comm_send(kr_ctx* c, const void* dev, size_t bytes, int peer) {
    kr_comm* m = c->comm;
    m->n_p2p++;
    if (m->rccl) {
        if (bytes) NCCLCHK(c, ncclSend(dev, bytes, ncclUint8, peer, m->nccl, c->stream));
        return KR_OK;
    }
    // (file transport: what the context's stream has queued for this buffer -- a merge, the header's copy -- is waited
    // for here; over RCCL the send is queued on that stream behind it.  Not counted: the rehearsal's own cost)
    std::vector<uint8_t> h(bytes);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bytes) HIPCHK(c, hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
    return file_put(c, h.data(), bytes, peer);
}
static int comm_recv(kr_ctx* c, void* dev, size_t bytes, int peer) {
    kr_comm* m = c->comm;
    m->n_p2p++;
    if (m->rccl) {
        if (bytes) NCCLCHK(c, ncclRecv(dev, bytes, ncclUint8, peer, m->nccl, c->stream));
        return KR_OK;
    }
    std::vector<uint8_t> h(bytes);
    int rc = file_get(c, h.data(), bytes, peer);
    if (rc) return rc;
    if (bytes) HIPCHK(c, hipMemcpy(dev, h.data(), bytes, hipMemcpyHostToDevice));
    return KR_OK;
}
// ---- small reductions over all ranks (n <= 8 doubles): op 0 = sum, 1 = max; result on every rank
int kr_comm_allreduce(kr_ctx* c, double* vals, int n, int op) {
    if (!c || !vals || n < 1 || n > 8 || (op != 0 && op != 1)) return fail(c, KR_ERR_PARAM, "kr_comm_allreduce: 1..8 values, op 0 | 1");
    if (!c->comm || c->comm->world == 1) return KR_OK;
    kr_comm* m = c->comm;
    COMM_ALIVE(c, "kr_comm_allreduce");
    WatchScope ws(c, "kr_comm_allreduce");
    HIPCHK(c, hipSetDevice(c->device));
    m->n_coll++;
    if (m->rccl) {
        double* d = (double*)m->scratch.p;
        HIPCHK(c, hipMemcpyAsync(d, vals, n * 8, hipMemcpyHostToDevice, c->stream));
        NCCLCHK(c, ncclAllReduce(d, d + 8, n, ncclDouble, op ? ncclMax : ncclSum, m->nccl, c->stream));
        HIPCHK(c, hipMemcpyAsync(vals, d + 8, n * 8, hipMemcpyDeviceToHost, c->stream));
        return comm_sync(c);
    }
    m->n_sync++;          // (file transport: the round trip through rank 0 stands for the synchronisation)
    // file transport: gather on rank 0, reduce, send back
    int rc;
    if (m->rank == 0) {
        std::vector<double> in(n);
        for (int r = 1; r < m->world; r++) {
            if ((rc = file_get(c, in.data(), n * 8, r))) return rc;
            for (int i = 0; i < n; i++) vals[i] = op ? std::max(vals[i], in[i]) : vals[i] + in[i];
        }
        for (int r = 1; r < m->world; r++)
            if ((rc = file_put(c, vals, n * 8, r))) return rc;
        return KR_OK;
    }
    if ((rc = file_put(c, vals, n * 8, 0))) return rc;
    return file_get(c, vals, n * 8, 0);
}

static int comm_agree(kr_ctx* c, int rc, const char* what);

// ---- n bytes of every rank -> all ranks (out[r n .. (r + 1) n) = rank r's; the same n everywhere).  For the small
// side data of the flow (the windows with IUPAC letters every rank found in its genomes: krisp_fasta.py), not for
// candidate lists.  RCCL: one all-gather between device buffers; file transport: every rank leaves its bytes for
// every other.
int kr_comm_allgather(kr_ctx* c, const void* mine, size_t n, void* out) {
    if (!c || (n && (!mine || !out))) return fail(c, KR_ERR_PARAM, "kr_comm_allgather: null buffer");
    const int world = c->comm ? c->comm->world : 1, rank = c->comm ? c->comm->rank : 0;
    if (n == 0) return KR_OK;
    if (world == 1) { memcpy(out, mine, n); return KR_OK; }
    kr_comm* m = c->comm;
    COMM_ALIVE(c, "kr_comm_allgather");
    WatchScope ws(c, "kr_comm_allgather");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (m->rccl) {
        if ((rc = comm_agree(c, ensure(c, m->gather, n * ((size_t)world + 1)), "kr_comm_allgather"))) return rc;
        uint8_t* d = (uint8_t*)m->gather.p;
        HIPCHK(c, hipMemcpyAsync(d, mine, n, hipMemcpyHostToDevice, c->stream));
        m->n_coll++;
        NCCLCHK(c, ncclAllGather(d, d + n, n, ncclUint8, m->nccl, c->stream));
        HIPCHK(c, hipMemcpyAsync(out, d + n, n * (size_t)world, hipMemcpyDeviceToHost, c->stream));
        return comm_sync(c);
    }
    m->n_coll++;
    m->n_sync++;
    for (int r = 0; r < world; r++)
        if (r != rank && (rc = file_put(c, mine, n, r))) return rc;
    for (int r = 0; r < world; r++) {
        if (r == rank) memcpy((uint8_t*)out + (size_t)r * n, mine, n);
        else if ((rc = file_get(c, (uint8_t*)out + (size_t)r * n, n, r))) return rc;
    }
    return KR_OK;
}

int kr_comm_barrier(kr_ctx* c) {
    if (!c) return KR_ERR_PARAM;
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rcj = join_lanes(c);
        if (rcj) return rcj;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double one = 1.0;
    return kr_comm_allreduce(c, &one, 1, 0);
}

// ---- all-or-none.  ncclSend / ncclRecv have no timeout: nothing may fail BETWEEN two matched calls and leave the
// partner inside one.  Round 5 (VERDICT r4 item 5): a round of the tree is ONE matched pair -- a message of a size all
// ranks agreed on before the tree starts, the list followed by a header {entries that count, poison} -- so there is no
// "count, then the list it announces" for a failure to fall between:
//   (1) exchange_prepare: ONE all-reduce (max) of {local candidate count, "I have failed", -room in my buffers}.  Nobody
//       enters the tree when a rank has failed already; the largest local count bounds every list that will travel
//       (a merge only shortens a list), so every rank knows the message size and whether every rank already has room
//       for it.  Only when some rank must grow its buffers do all ranks grow and agree once more (the first exchange
//       of a context; afterwards the buffers fit).
//   (2) a rank whose merge fails mid-tree keeps its place, sends its message with the poison word set, and returns its
//       error when its last matched call is behind it; the poison reaches rank 0 and travels on with the broadcast.
//   (3) a receiver launches the merge without having seen the count (k_cands_flag reads it from the header on the device)
//       and learns count, poison and result with ONE synchronisation per round; a sender does not synchronise at all.
// Per step on rank 0 at world 8: 1 (prepare) + 3 (rounds) + 1 (the broadcast's own prepare; rank 0 is its root and does not
// wait for it) = 5 host synchronisations, 2 all-reduces + 3 receives + 1 broadcast (round 4: 13 blocking calls with a
// synchronisation each); kr_debug_comm counts them.
#define COMM_POISON (~0ull)
static int comm_agree(kr_ctx* c, int rc, const char* what) {
    if (!c->comm || c->comm->world <= 1) return rc;
    const std::string mine = rc < 0 ? c->err : std::string();
    double bad = rc < 0 ? 1.0 : 0.0;
    const int rca = kr_comm_allreduce(c, &bad, 1, 1);
    if (rc < 0) { c->err = mine; g_last_error = mine; return rc; }
    if (rca) return rca;
    if (bad > 0) return fail(c, KR_ERR_STATE, "%s: another rank failed", what);
    return KR_OK;
}

// ---- the exchange step.  Every rank holds the candidates of its own genomes (kr_intersect;
// unfiltered, or already pruned with the diagnostic filter: "some column has disjoint ingroup /
// outgroup base sets" is monotone -- masks only grow under merging -- so a candidate that fails
// it on partial masks fails it globally and may be dropped at any stage).  Afterwards rank 0
// holds the candidates present on EVERY rank, masks OR-ed (and filtered when apply_filter); the
// other ranks' sets are spent.  ceil(log2 world) rounds of distinct pairs; the lists go from
// device buffer to device buffer and are merged on the device (k_cands_flag / k_cands_compact).
// Returns the final count on rank 0 and 0 elsewhere (those sets are spent).
// capacity (entries) of this rank's three candidate buffers beyond the two entries of slack the header lives in
static u64 ex_room(const kr_ctx* c) {
    const size_t b = std::min(c->candA.bytes, std::min(c->candB.bytes, c->other.bytes)) / sizeof(kr_cand);
    return b >= 2 ? (u64)b - 2 : 0;
}
// (1) above.  local_rc < 0: this rank has failed already (its error text is kept); my_count = the entries of the list this
// rank may send.  Leaves c->ex_cap.  Every rank of a collective call makes the same calls here whatever it holds: what a
// rank did to its own candidate set since the last exchange must not decide whether it enters a collective.
static int exchange_prepare(kr_ctx* c, int local_rc, const char* what, u64 my_count) {
    if (local_rc >= 0) {
        // (room for a header even when no rank holds a candidate: a message is never shorter than that)
        int rc0 = ensure(c, c->other, 64);
        if (!rc0) rc0 = ensure(c, c->candB, 64);
        if (!rc0) rc0 = ensure(c, c->candA, 64);
        if (rc0) local_rc = rc0;
    }
    const std::string mine = local_rc < 0 ? c->err : std::string();
    const u64 have = c->ncand > 0 ? (u64)c->ncand : 0;              // (live entries of candB, kept when it grows)
    double v[3] = {(double)my_count, local_rc < 0 ? 1.0 : 0.0, -(double)ex_room(c)};       // (counts < 2^53: exact)
    const int rca = kr_comm_allreduce(c, v, 3, 1);
    if (local_rc < 0) { c->err = mine; g_last_error = mine; return local_rc; }
    if (rca) return rca;
    if (v[1] > 0) return fail(c, KR_ERR_STATE, "%s: another rank failed", what);
    const u64 cap = (u64)v[0], room = (u64)(-v[2]);
    if (room < cap) {
        int rc = ensure(c, c->other, (size_t)(cap + 2) * sizeof(kr_cand));
        if (!rc) rc = ensure_keep(c, c->candB, (size_t)(cap + 2) * sizeof(kr_cand), (size_t)have * sizeof(kr_cand));
        if (!rc) rc = ensure(c, c->candA, (size_t)(cap + 2) * sizeof(kr_cand));
        if ((rc = comm_agree(c, rc, what))) return rc;
    }
    c->ex_cap = cap;
    return KR_OK;
}
// candidates := candidates INTERSECT the list just received into c->other (ex_cap entries of room, then its header),
// masks OR-ed, the filter applied: the count is read on the device; count, poison and result reach the host with the
// one synchronisation at the end
static int64_t cands_merge_incoming(kr_ctx* c, int apply_filter) {
    kr_comm* m = c->comm;
    const u32 n = (u32)std::max<int64_t>(c->ncand, 0);
    const u64* hdr = (const u64*)((const char*)c->other.p + (size_t)c->ex_cap * sizeof(kr_cand));
    hipStream_t st = c->stream;
    const u32 nblk = (n + 255) / 256;
    int rc = KR_OK;
    u32 total = 0;
    if (n) {
        rc = cands_compact_room(c, n);          // (candA: sized by exchange_prepare already)
        if (!rc) {
            StageScope sc(c, KR_ST_MERGE);
            hipLaunchKernelGGL(k_cands_flag, dim3(nblk), dim3(256), 0, st, (kr_cand*)c->candB.p, n, (const kr_cand*)c->other.p, 0u,
                               1, fmode(c, apply_filter), c->g.D, (u32*)c->flags.p, (u32*)c->blockcnt.p, hdr);
            HIPCHK(c, hipMemcpyAsync(&total, cands_compact_enqueue(c, n, st, false), 4, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(c, hipMemcpyAsync(m->hdr_in, hdr, 16, hipMemcpyDeviceToHost, st));
    int rs = comm_sync(c);                       // (also when the merge could not be launched: the receive is behind us)
    if (rs) return rs;
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    if (n) cands_compact_adopt(c, total);
    return c->ncand;
}

int64_t kr_cands_reduce(kr_ctx* c, int apply_filter) {
    if (!c || !c->comm) return fail(c, KR_ERR_STATE, "kr_comm_init first");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    const auto t0 = std::chrono::steady_clock::now();
    m->n_reduce++;
    int rc;
    if (m->world == 1) {
        if (c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
        return apply_filter ? cands_merge_device(c, 0, 0, 1) : c->ncand;
    }
    COMM_ALIVE(c, "kr_cands_reduce");
    WatchScope ws(c, "kr_cands_reduce");
    if ((rc = exchange_prepare(c, c->ncand < 0 ? fail(c, KR_ERR_STATE, "no candidate set") : 0, "kr_cands_reduce",
                               c->ncand > 0 ? (u64)c->ncand : 0)))
        return rc;
    const size_t msg = (size_t)c->ex_cap * sizeof(kr_cand) + 16;
    int err = 0;
    std::string errmsg;
    auto poison = [&](int code) { if (!err) { err = code; errmsg = c->err; } };
    bool active = true;
    for (int step = 1; step < m->world; step *= 2) {
        if (!active) continue;
        if (m->rank % (2 * step) == 0) {
            const int partner = m->rank + step;
            if (partner >= m->world) continue;
            if ((rc = comm_recv(c, c->other.p, msg, partner))) return rc;      // (the transport itself: nothing left to save)
            const int64_t left = cands_merge_incoming(c, apply_filter);
            if (m->hdr_in[1]) poison(fail(c, KR_ERR_STATE, "kr_cands_reduce: rank %d failed", partner));
            else if (left < 0) poison((int)left);
        } else {
            const int partner = m->rank - step;
            active = false;
            m->hdr_out[0] = err ? 0 : (u64)c->ncand;
            m->hdr_out[1] = err ? 1 : 0;
            HIPCHK(c, hipMemcpyAsync((char*)c->candB.p + (size_t)c->ex_cap * sizeof(kr_cand), m->hdr_out, 16, hipMemcpyHostToDevice, c->stream));
            if ((rc = comm_send(c, c->candB.p, msg, partner))) return rc;      // (no synchronisation: what follows on the stream is ordered)
        }
    }
    m->ex_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (err) {
        // (rank 0's failure reaches the others with the broadcast's header; any other rank's reached rank 0 above)
        c->err = errmsg; g_last_error = errmsg;
        if (m->rank == 0) c->ncand = -1;
        return err;
    }
    if (m->rank != 0) {
        c->ncand = 0;
        return 0;
    }
    return c->ncand;        // (rank 0's last merge saw every rank's masks and applied the filter)
}

// rank 0's candidates -> every rank's candidate set (for the local collect).  Returns the count.
int64_t kr_cands_bcast(kr_ctx* c) {
    if (!c || !c->comm) return fail(c, KR_ERR_STATE, "kr_comm_init first");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    if (m->world == 1) return c->ncand;
    COMM_ALIVE(c, "kr_cands_bcast");
    WatchScope ws(c, "kr_cands_bcast");
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    // (the ranks agree on the message size and on "nobody has failed" again: rank 0 may hold another list than the one the
    // reduction left -- kr_cands_load, the wide path's lists --, and no rank may decide that from what it holds itself)
    const bool root_failed = m->rank == 0 && c->ncand < 0;
    if ((rc = exchange_prepare(c, root_failed ? fail(c, KR_ERR_STATE, "no candidate set") : 0, "kr_cands_bcast",
                               m->rank == 0 && c->ncand > 0 ? (u64)c->ncand : 0)))
        return rc;
    const size_t off = (size_t)c->ex_cap * sizeof(kr_cand), msg = off + 16;
    if (m->rank == 0) {
        // (a root whose reduction failed still broadcasts: the poison word tells every rank)
        m->hdr_out[0] = root_failed ? 0 : (u64)c->ncand;
        m->hdr_out[1] = root_failed ? 1 : 0;
        HIPCHK(c, hipMemcpyAsync((char*)c->candB.p + off, m->hdr_out, 16, hipMemcpyHostToDevice, c->stream));
    }
    if (m->rccl) {
        m->n_coll++;
        NCCLCHK(c, ncclBroadcast(c->candB.p, c->candB.p, msg, ncclUint8, 0, m->nccl, c->stream));
    } else if (m->rank == 0) {
        for (int r = 1; r < m->world; r++)
            if ((rc = comm_send(c, c->candB.p, msg, r))) return rc;
    } else {
        if ((rc = comm_recv(c, c->candB.p, msg, 0))) return rc;
    }
    if (m->rank != 0) {
        HIPCHK(c, hipMemcpyAsync(m->hdr_in, (const char*)c->candB.p + off, 16, hipMemcpyDeviceToHost, c->stream));
        if ((rc = comm_sync(c))) return rc;
        if (m->hdr_in[1]) { c->ncand = -1; return fail(c, KR_ERR_STATE, "kr_cands_bcast: rank 0 failed"); }
        c->ncand = (int64_t)m->hdr_in[0];
    }
    m->ex_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (root_failed) return fail(c, KR_ERR_STATE, "no candidate set");
    return c->ncand;
}

// every rank's records (kr_collect) -> rank 0's record buffer, rank order (kr_fetch then returns them all).  Returns
// the total on rank 0, the local count elsewhere.  One all-gather of the counts, one agreement that rank 0 has room,
// then every rank sends and rank 0 receives without a word in between (three synchronisations whatever the world).
int64_t kr_records_gather(kr_ctx* c) {
    if (!c || !c->comm) return fail(c, KR_ERR_STATE, "kr_comm_init first");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    if (m->world == 1) return c->nrecords;
    COMM_ALIVE(c, "kr_records_gather");
    WatchScope ws(c, "kr_records_gather");
    int rc;
    const u64 mine = c->nrecords > 0 ? (u64)c->nrecords : 0;
    std::vector<u64> all((size_t)m->world, 0);
    if ((rc = kr_comm_allgather(c, &mine, 8, all.data()))) return rc;
    rc = KR_OK;
    if (m->rank == 0) {
        u64 total = 0;
        for (u64 x : all) total += x;
        rc = ensure_keep(c, c->records, (size_t)(total + 2) * sizeof(kr_record), (size_t)mine * sizeof(kr_record));
    }
    if ((rc = comm_agree(c, rc, "kr_records_gather"))) return rc;
    if (m->rank != 0) {
        if ((rc = comm_send(c, c->records.p, (size_t)mine * sizeof(kr_record), 0))) return rc;
        return c->nrecords;
    }
    u64 at = mine;
    for (int r = 1; r < m->world; r++) {
        if ((rc = comm_recv(c, (kr_record*)c->records.p + at, (size_t)all[r] * sizeof(kr_record), r))) return rc;
        at += all[r];
    }
    if ((rc = comm_sync(c))) return rc;
    c->nrecords = (int64_t)at;
    return c->nrecords;
}

// One round of the tree with the rank itself as its partner, over RCCL (any world size, every rank calls it): the candidate
// list with its header travels from candB to `other` through ncclSend / ncclRecv (grouped: a self pair must be), and is merged
// as a received list is -- the count read from the header on the device, masks OR-ed, the filter, one synchronisation.  What
// a box with ONE GPU can show of the exchange on the real transport (the tree itself needs peers: file transport in the
// tests): the message layout, the device-side count, the merge behind a receive.  Returns the count, which equals the
// count before for an unfiltered list (every prefix meets itself).
int64_t kr_debug_cands_selfexchange(kr_ctx* c, int apply_filter) {
    if (!c || !c->comm || !c->comm->rccl) return fail(c, KR_ERR_STATE, "kr_debug_cands_selfexchange: needs an RCCL communicator");
    if (c->ncand < 0) return fail(c, KR_ERR_STATE, "no candidate set");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    COMM_ALIVE(c, "kr_debug_cands_selfexchange");
    WatchScope ws(c, "kr_debug_cands_selfexchange");
    int rc;
    // (the agreement: with one rank it is its own maximum; with several the all-reduce of exchange_prepare)
    if (m->world > 1) {
        if ((rc = exchange_prepare(c, 0, "kr_debug_cands_selfexchange", (u64)c->ncand))) return rc;
    } else {
        const u64 cap = (u64)c->ncand;
        if ((rc = ensure(c, c->other, (size_t)(cap + 2) * sizeof(kr_cand)))) return rc;
        if ((rc = ensure_keep(c, c->candB, (size_t)(cap + 2) * sizeof(kr_cand), (size_t)cap * sizeof(kr_cand)))) return rc;
        if ((rc = ensure(c, c->candA, (size_t)(cap + 2) * sizeof(kr_cand)))) return rc;
        c->ex_cap = cap;
    }
    const size_t off = (size_t)c->ex_cap * sizeof(kr_cand), msg = off + 16;
    m->hdr_out[0] = (u64)c->ncand;
    m->hdr_out[1] = 0;
    HIPCHK(c, hipMemcpyAsync((char*)c->candB.p + off, m->hdr_out, 16, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, ncclGroupStart());
    NCCLCHK(c, ncclSend(c->candB.p, msg, ncclUint8, m->rank, m->nccl, c->stream));
    NCCLCHK(c, ncclRecv(c->other.p, msg, ncclUint8, m->rank, m->nccl, c->stream));
    NCCLCHK(c, ncclGroupEnd());
    m->n_p2p += 2;
    const int64_t left = cands_merge_incoming(c, apply_filter);
    if (left < 0) return left;
    if (m->hdr_in[0] != m->hdr_out[0] || m->hdr_in[1] != 0)
        return fail(c, KR_ERR_HIP, "kr_debug_cands_selfexchange: header came back as {%llu, %llu}", (unsigned long long)m->hdr_in[0],
                    (unsigned long long)m->hdr_in[1]);
    return left;
}

// what one blocking call of the exchange costs on this box (microseconds, host clock, averaged over reps): out[0] an
// all-reduce of three doubles + synchronisation (exchange_prepare), out[1] a send / receive pair of `bytes` to the rank
// itself + synchronisation (a round of the tree: the message and the wait for it; between two GPUs the wire time of the
// message comes on top), out[2] a broadcast of `bytes` + synchronisation.  RCCL only (a communicator of any world size;
// every rank calls it).  The per-call price list behind the budget of h_comm.inc's header: bench.py --force-comm prints it.
int kr_debug_comm_probe(kr_ctx* c, size_t bytes, int reps, double* out3) {
    if (!c || !out3 || reps < 1) return KR_ERR_PARAM;
    if (!c->comm || !c->comm->rccl) return fail(c, KR_ERR_STATE, "kr_debug_comm_probe: needs an RCCL communicator");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    COMM_ALIVE(c, "kr_debug_comm_probe");
    WatchScope ws(c, "kr_debug_comm_probe");
    DevBuf a, b;
    struct Guard {              // (every exit gives the two buffers back: ADVICE r5)
        kr_ctx* c; DevBuf &a, &b;
        ~Guard() { (void)hipStreamSynchronize(c->stream); release(c, a); release(c, b); }
    } guard{c, a, b};
    int rc;
    if ((rc = ensure(c, a, bytes + 64)) || (rc = ensure(c, b, bytes + 64))) return rc;
    HIPCHK(c, hipMemsetAsync(a.p, 0, bytes + 64, c->stream));
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1, int n) {
        return std::chrono::duration<double, std::micro>(t1 - t0).count() / n;
    };
    double v[3] = {1, 2, 3};
    if ((rc = kr_comm_allreduce(c, v, 3, 1))) return rc;           // warm-up (the first collective builds its channels)
    auto t0 = now();
    for (int r = 0; r < reps; r++) {
        if (m->world > 1) { if ((rc = kr_comm_allreduce(c, v, 3, 1))) return rc; }
        else {
            double* d = (double*)m->scratch.p;
            NCCLCHK(c, ncclAllReduce(d, d + 8, 3, ncclDouble, ncclMax, m->nccl, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    out3[0] = us(t0, now(), reps);
    const int peer = m->rank;                                       // (to itself: the call path without the wire)
    for (int r = -1; r < reps; r++) {
        if (r == 0) t0 = now();
        NCCLCHK(c, ncclGroupStart());
        NCCLCHK(c, ncclSend(a.p, bytes, ncclUint8, peer, m->nccl, c->stream));
        NCCLCHK(c, ncclRecv(b.p, bytes, ncclUint8, peer, m->nccl, c->stream));
        NCCLCHK(c, ncclGroupEnd());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    out3[1] = us(t0, now(), reps);
    for (int r = -1; r < reps; r++) {
        if (r == 0) t0 = now();
        NCCLCHK(c, ncclBroadcast(a.p, a.p, bytes, ncclUint8, 0, m->nccl, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    out3[2] = us(t0, now(), reps);
    return KR_OK;
}

// test aid for the watchdog on the real transport (any world size; at world 1 the rank is its own silent partner): a receive
// nobody will ever send to, then the synchronisation an exchange round ends with.  The watchdog's deadline (kr_comm_set_timeout)
// passes, it aborts the communicator, the synchronisation returns and this call with KR_ERR_STATE -- or RCCL refuses the
// unmatched receive outright (KR_ERR_HIP).  The communicator is spent either way.  Returns KR_OK only if the receive completed.
int kr_debug_comm_hang(kr_ctx* c) {
    if (!c || !c->comm || !c->comm->rccl) return fail(c, KR_ERR_STATE, "kr_debug_comm_hang: needs an RCCL communicator");
    HIPCHK(c, hipSetDevice(c->device));
    kr_comm* m = c->comm;
    COMM_ALIVE(c, "kr_debug_comm_hang");
    WatchScope ws(c, "kr_debug_comm_hang (a receive without a sender)");
    NCCLCHK(c, ncclRecv((char*)m->scratch.p + 64, 8, ncclUint8, (m->rank + 1) % m->world, m->nccl, c->stream));
    return comm_sync(c);
}

// what the exchange has cost this context so far: out[0] host synchronisations, [1] point-to-point calls, [2] collectives
// (all-reduce, all-gather, broadcast), [3] microseconds inside kr_cands_reduce / kr_cands_bcast, [4] kr_cands_reduce
// calls, [5] entries of the agreed message size; out[6..7] = 0
int kr_debug_comm(kr_ctx* c, int64_t* out8) {
    if (!c || !out8) return KR_ERR_PARAM;
    for (int i = 0; i < 8; i++) out8[i] = 0;
    if (!c->comm) return KR_OK;
    out8[0] = c->comm->n_sync;
    out8[1] = c->comm->n_p2p;
    out8[2] = c->comm->n_coll;
    out8[3] = (int64_t)c->comm->ex_us;
    out8[4] = c->comm->n_reduce;
    out8[5] = (int64_t)c->ex_cap;
    return KR_OK;
}
