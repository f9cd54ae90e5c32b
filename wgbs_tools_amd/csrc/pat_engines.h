// pat_engines.h — the engines that take pat text in chunks (wgbsseg_patbeta, wgbsseg_homog, wgbsseg_fraglen, wgbsseg_bimodal, wgbsseg_patview) and the one that takes BED
// text the same way (wgbsseg_bedbeta) and the one that takes FASTA text cut at any byte (wgbsseg_fasta, at the end), the feed they share
// (PatFeed, PrevRead), the stand-alone wgbsseg_bgzf_inflate and their extern "C" entry points.  Part of wgbsseg.hip, which includes it once set_err, HIP_TRY, check_device and the owners are
// in scope; what an engine decides on the host is in homog_plan.h, frag_plan.h, bimodal_plan.h, view_plan.h and bed2beta_plan.h, this file stages, launches and fetches.
#pragma once

// The pat-text feed of an engine (wgbsseg_patbeta / _homog / _fraglen / _bimodal / _patview): one device and stream; text chunks through two page-locked
// staging buffers and two device buffers, so that the caller's decompression of chunk k+1 overlaps the copy and the kernels of
// chunk k; the input offset of the next chunk; and the device time of the launches the engine brackets with span_begin / span_end.
// There are two ways to fill text[k]: stage_chunk copies text the caller inflated; stage_bgzf copies BGZF bytes as they lie in the file
// (with their member table, inflate_plan.h) and has k_bgzf_inflate write the members' text behind the carry — the end of the call
// before, from its last newline on, which is kept on the host.  Everything behind the staging is the same for both.
// Teardown: an engine's buffers — its own and the feed's — must not go while the stream may still use them.  Members go in reverse order of
// declaration and an engine's `feed` comes first, so declaration order alone would free the engine's buffers before the feed had a say: every
// engine's destructor calls drain() instead (explicit, one line each), and so does the feed's own for the buffers it holds itself.
struct PatFeed {
    enum { LAUNCHES = 0, INFLATE = 1 };                           // the two timed spans: the engine's launches, k_bgzf_inflate
    enum { TEXT = 1, BGZF = 2 };                                  // what the engine is fed (one of the two, once it has been fed)
    int device = 0;
    Stream st;                                                    // (declared first: goes last)
    PinnedBuf stage[2];
    DevBuf text[2];
    PinnedBuf cstage[2];                                          // BGZF: the member table, the compressed bytes, the carry
    DevBuf comp[2];                                               //       the member table and the compressed bytes
    DevBuf bad_member;                                            //       (file offset << 8 | reason) of the first member refused, ~0: none
    std::string carry;                                            //       the text behind the last newline of the calls so far
    unsigned long long file_off = 0;                              //       BGZF bytes consumed so far
    int mode = 0;
    Event ev[2];                                                  // after the work on slot k's text
    bool busy[2] = {false, false};
    int k = 0;                                                    // the slot of the next chunk
    unsigned long long fed = 0;                                   // bytes fed so far
    double span_ms[2] = {0.0, 0.0};                               // the spans read so far
    std::deque<std::pair<Event, Event>> spans[2];                 // recorded, in stream order, not read yet
    std::vector<Event> spare;                                     // the events of read spans, for the next ones

    int open(int dev, char* err, size_t errlen)
    {
        const int rc = check_device(dev, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        device = dev;
        HIP_TRY(st.create());
        for (auto& e : ev) HIP_TRY(e.create(false));
        return WGBSSEG_OK;
    }
    void drain()                                                  // the stream has passed everything queued on it, the spans are read: buffers may go
    {
        (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        collect();
    }
    ~PatFeed() { drain(); }
    int claim(int want, const char* name, char* err, size_t errlen)
    {
        if (mode && mode != want) { set_err(err, errlen, "%s: feed and feed_bgzf cannot be mixed on one engine", name); return WGBSSEG_E_ARG; }
        mode = want;
        return WGBSSEG_OK;
    }
    // the checks of a feed call: -1 when refused (err set), 0 for an empty chunk, else the chunk's number of tiles
    static int64_t tiles(const char* name, const void* engine, const char* text, int64_t n_bytes, char* err, size_t errlen)
    {
        if (!engine || (n_bytes && !text) || n_bytes < 0) { set_err(err, errlen, "bad arguments to %s_feed", name); return -1; }
        if (n_bytes == 0) return 0;
        if (text[n_bytes - 1] != '\n') { set_err(err, errlen, "%s_feed: a chunk must end with a complete line", name); return -1; }
        return tiles_of(name, n_bytes, err, errlen);
    }
    static int64_t tiles_of(const char* name, int64_t n_bytes, char* err, size_t errlen)
    {
        const int64_t gx = (n_bytes + WG_PAT_TILE - 1) / WG_PAT_TILE;     // one workgroup per tile of text
        if (gx > 0x7fffffff) { set_err(err, errlen, "%s_feed: chunk too large", name); return -1; }
        return gx;
    }
    // waits until the chunk before last (same slot) has been consumed, then queues the copy of this one; *dev: its device copy
    int stage_chunk(const char* host, int64_t n_bytes, const char** dev, char* err, size_t errlen)
    {
        if (busy[k]) { HIP_TRY(hipEventSynchronize(ev[k])); collect(); }
        if (!stage[k].ensure((size_t)n_bytes)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
        HIP_TRY(text[k].ensure((size_t)n_bytes));
        memcpy(stage[k].p, host, (size_t)n_bytes);
        HIP_TRY(hipMemcpyAsync(text[k].p, stage[k].p, (size_t)n_bytes, hipMemcpyHostToDevice, st));
        *dev = text[k].as<char>();
        return WGBSSEG_OK;
    }
    // the same for a planned BGZF call: the member table and the compressed bytes to comp[k], the carry to the front of text[k],
    // k_bgzf_inflate (a timed span of its own) for the members' text behind it
    int stage_bgzf(const void* bytes, const BgzfPlan& p, const char** dev, char* err, size_t errlen)
    {
        if (busy[k]) { HIP_TRY(hipEventSynchronize(ev[k])); collect(); }
        const size_t tb = (size_t)p.n_dev * sizeof(wg_bgzf_member), cb = (size_t)p.comp_bytes, cin = (size_t)p.carry_in;
        if (!cstage[k].ensure(tb + cb + cin)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
        HIP_TRY(comp[k].ensure(tb + cb));
        HIP_TRY(text[k].ensure((size_t)p.text_cap));
        if (!bad_member.p) { HIP_TRY(bad_member.ensure(8)); HIP_TRY(hipMemsetAsync(bad_member.p, 0xff, 8, st)); }
        char* host = static_cast<char*>(cstage[k].p);
        memcpy(host, p.members.data(), tb);
        memcpy(host + tb, bytes, cb);
        memcpy(host + tb + cb, carry.data(), cin);
        HIP_TRY(hipMemcpyAsync(comp[k].p, host, tb + cb, hipMemcpyHostToDevice, st));
        if (cin) HIP_TRY(hipMemcpyAsync(text[k].p, host + tb + cb, cin, hipMemcpyHostToDevice, st));
        HIP_TRY(span_begin(INFLATE));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)((p.n_dev + WG_INF_WAVES - 1) / WG_INF_WAVES)), dim3(64 * WG_INF_WAVES), 0, st,
                           comp[k].as<uint8_t>() + tb, comp[k].as<wg_bgzf_member>(), p.n_dev, text[k].as<uint8_t>(), bad_member.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(span_end(INFLATE));
        *dev = text[k].as<char>();
        return WGBSSEG_OK;
    }
    // the chunk's work has been queued: the slot is busy until the stream passes here
    hipError_t chunk_queued(int64_t n_bytes)
    {
        const hipError_t e = hipEventRecord(ev[k], st);
        busy[k] = true;
        k ^= 1;
        fed += (unsigned long long)n_bytes;
        return e;
    }
    hipError_t span_begin(int which = LAUNCHES)
    {
        Event e[2];
        for (auto& x : e) {
            if (!spare.empty()) { x = std::move(spare.back()); spare.pop_back(); continue; }
            const hipError_t r = x.create();
            if (r != hipSuccess) return r;
        }
        spans[which].emplace_back(std::move(e[0]), std::move(e[1]));
        return hipEventRecord(spans[which].back().first, st);
    }
    hipError_t span_end(int which = LAUNCHES) { return hipEventRecord(spans[which].back().second, st); }
    // A staged chunk of an engine whose chunk is one launch: stage(&device text) (the chunk's copy, either way), `before` (untimed stream
    // work in front of the launch), then launch(tiles, device text) as one timed span.
    template <class Engine, class Stage, class Before, class Launch>
    static int one_launch(Engine* e, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen, Before&& before, Launch&& launch)
    {
        PatFeed& f = e->feed;
        HIP_TRY(hipSetDevice(f.device));
        const char* dtext = nullptr;
        const int rc = stage(&dtext);
        if (rc != WGBSSEG_OK) return rc;
        HIP_TRY(before());
        HIP_TRY(f.span_begin());
        launch((unsigned)gx, dtext);
        HIP_TRY(hipGetLastError());
        HIP_TRY(f.span_end());
        HIP_TRY(f.chunk_queued(n_bytes));
        return WGBSSEG_OK;
    }
    // A feed call with text: the checks, then pat_chunk(engine, n_bytes, tiles, stage, err, errlen) — the engine's work on a chunk that stage() puts on the
    // device: an overload per engine, declared behind it and found here by argument-dependent lookup.  Engine::name begins the messages.  Not called for a chunk that is refused or empty.
    template <class Engine>
    static int feed_text(Engine* e, const char* host, int64_t n_bytes, char* err, size_t errlen)
    {
        const int64_t gx = tiles(Engine::name, e, host, n_bytes, err, errlen);
        if (gx <= 0) return gx < 0 ? WGBSSEG_E_ARG : WGBSSEG_OK;
        PatFeed& f = e->feed;
        const int rc = f.claim(TEXT, Engine::name, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        return pat_chunk(e, n_bytes, gx, [&](const char** dev) { return f.stage_chunk(host, n_bytes, dev, err, errlen); }, err, errlen);
    }
    // A feed call with BGZF bytes: the plan (members, line rule), then the same pat_chunk over the complete lines of carry + members, staged
    // by stage_bgzf; the text behind the last newline becomes the carry.  *consumed: the bytes of the complete members.
    template <class Engine>
    static int feed_bgzf(Engine* e, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
    {
        if (!e || !consumed || n_bytes < 0 || (n_bytes && !bytes)) { set_err(err, errlen, "bad arguments to %s_feed_bgzf", Engine::name); return WGBSSEG_E_ARG; }
        *consumed = 0;
        PatFeed& f = e->feed;
        int rc = f.claim(BGZF, Engine::name, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        BgzfPlan p;
        std::string msg;
        rc = plan_bgzf(static_cast<const uint8_t*>(bytes), n_bytes, f.file_off, f.carry, p, msg);
        if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
        if (p.n_text > 0) {
            const int64_t gx = tiles_of(Engine::name, p.n_text, err, errlen);
            if (gx < 0) return WGBSSEG_E_ARG;
            HIP_TRY(hipSetDevice(f.device));
            rc = pat_chunk(e, p.n_text, gx, [&](const char** dev) { return f.stage_bgzf(bytes, p, dev, err, errlen); }, err, errlen);
            if (rc != WGBSSEG_OK) return rc;
        }
        f.carry = std::move(p.carry);
        f.file_off += (unsigned long long)p.consumed;
        *consumed = p.consumed;
        return WGBSSEG_OK;
    }
    // finish(): a last line without its newline is still in the carry; it is fed as text, with the newline (as pat_chunks does)
    template <class Engine>
    static int flush_carry(Engine* e, char* err, size_t errlen)
    {
        if (e->feed.carry.empty()) return WGBSSEG_OK;
        std::string last;
        last.swap(e->feed.carry);
        last.push_back('\n');
        const int64_t n = (int64_t)last.size(), gx = tiles_of(Engine::name, n, err, errlen);
        if (gx < 0) return WGBSSEG_E_ARG;
        return pat_chunk(e, n, gx, [&](const char** dev) { return e->feed.stage_chunk(last.data(), n, dev, err, errlen); }, err, errlen);      // (copied before this returns)
    }
    // The byte-cut path (wgbsseg_fasta): a chunk may end anywhere, so there is no line check, no line rule and no host carry; what a
    // chunk leaves open is the engine's own business, on the device.  The same pat_chunk hook, staging and spans as above.
    template <class Engine>
    static int feed_bytes(Engine* e, const char* host, int64_t n_bytes, char* err, size_t errlen)
    {
        if (!e || (n_bytes && !host) || n_bytes < 0) { set_err(err, errlen, "bad arguments to %s_feed", Engine::name); return WGBSSEG_E_ARG; }
        if (n_bytes == 0) return WGBSSEG_OK;
        const int64_t gx = tiles_of(Engine::name, n_bytes, err, errlen);
        if (gx < 0) return WGBSSEG_E_ARG;
        PatFeed& f = e->feed;
        const int rc = f.claim(TEXT, Engine::name, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        return pat_chunk(e, n_bytes, gx, [&](const char** dev) { return f.stage_chunk(host, n_bytes, dev, err, errlen); }, err, errlen);
    }
    template <class Engine>
    static int feed_bgzf_bytes(Engine* e, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
    {
        if (!e || !consumed || n_bytes < 0 || (n_bytes && !bytes)) { set_err(err, errlen, "bad arguments to %s_feed_bgzf", Engine::name); return WGBSSEG_E_ARG; }
        *consumed = 0;
        PatFeed& f = e->feed;
        int rc = f.claim(BGZF, Engine::name, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        BgzfPlan p;
        std::string msg;
        rc = plan_bgzf_bytes(static_cast<const uint8_t*>(bytes), n_bytes, f.file_off, p, msg);
        if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
        if (p.n_text > 0) {
            const int64_t gx = tiles_of(Engine::name, p.n_text, err, errlen);
            if (gx < 0) return WGBSSEG_E_ARG;
            HIP_TRY(hipSetDevice(f.device));
            rc = pat_chunk(e, p.n_text, gx, [&](const char** dev) { return f.stage_bgzf(bytes, p, dev, err, errlen); }, err, errlen);
            if (rc != WGBSSEG_OK) return rc;
        }
        f.file_off += (unsigned long long)p.consumed;
        *consumed = p.consumed;
        return WGBSSEG_OK;
    }
    // finish(): a member k_bgzf_inflate refused comes before any refusal of the text.  Waits for the stream.
    int inflate_refused(char* err, size_t errlen)
    {
        if (!bad_member.p) return WGBSSEG_OK;
        unsigned long long bad = ~0ULL;
        HIP_TRY(hipMemcpyAsync(&bad, bad_member.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad == ~0ULL) return WGBSSEG_OK;
        std::string msg;
        (void)wg_inflate_refuse(msg, bad >> 8, (int)(bad & 0xff));
        set_err(err, errlen, "%s", msg.c_str());
        return WGBSSEG_E_ARG;
    }
    // adds the spans the stream has passed to span_ms (in order: the first one still running ends the walk)
    void collect()
    {
        for (int w = 0; w < 2; w++)
            while (!spans[w].empty()) {
                float ms = 0.f;
                const hipError_t e = hipEventElapsedTime(&ms, spans[w].front().first, spans[w].front().second);
                if (e == hipErrorNotReady) break;
                if (e == hipSuccess) span_ms[w] += (double)ms;
                spare.push_back(std::move(spans[w].front().first)); spare.push_back(std::move(spans[w].front().second));
                spans[w].pop_front();
            }
    }
    double kernel_ms(int which = LAUNCHES)                        // waits for the stream; -1 on a HIP error
    {
        if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1.0;
        collect();
        return span_ms[which];
    }
};

// the refusals of the input that the pat engines share, "<prefix> <what> at byte offset <off> ..."; false when off is ~0 (none)
enum class PatRefusal { bad_line, unsorted };
static bool pat_refused(PatRefusal why, unsigned long long off, const char* prefix, char* err, size_t errlen)
{
    if (off == ~0ULL) return false;
    if (why == PatRefusal::bad_line)
        set_err(err, errlen, "%s invalid line at byte offset %llu of the input (too few columns, or a site / count that is not a number)", prefix, off);
    else
        set_err(err, errlen, "%s the pat file is not sorted: the read at byte offset %llu of the input starts before the read before it", prefix, off);
    return true;
}

// The last read of the chunks so far (homog, fraglen and view refuse a descending read): two slots on the device, 16 bytes
struct PrevRead {
    DevBuf slots;
    unsigned long long chunks = 0;                               // chunks launched so far: the slots swap with each
    long long* in() const { return slots.as<long long>() + ((chunks & 1) ^ 1); }      // chunk c's kernel reads slot (c + 1) & 1 ...
    long long* out() const { return slots.as<long long>() + (chunks & 1); }           // ... and writes slot c & 1, which carry() has given in's value: kept when the chunk holds no read
    hipError_t carry(hipStream_t st) const { return hipMemcpyAsync(out(), in(), 8, hipMemcpyDeviceToDevice, st); }      // in front of a chunk's launch
    hipError_t reset() const                                     // no read yet (a blocking copy)
    {
        const long long none[2] = {WG_PAT_NO_SITE, WG_PAT_NO_SITE};
        return hipMemcpy(slots.p, none, sizeof(none), hipMemcpyHostToDevice);
    }
};

// pat -> beta accumulator: counts on one device; k_pat_count is timed.
struct wgbsseg_patbeta {
    static constexpr const char* name = "patbeta";
    PatFeed feed;
    int64_t start = 1, end = 1;
    DevBuf meth, cov, outb, bad;
    ~wgbsseg_patbeta() { feed.drain(); }
};

// a staged chunk of n_bytes / gx tiles: k_pat_count over it
template <class Stage>
static int pat_chunk(wgbsseg_patbeta* p, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    return PatFeed::one_launch(p, n_bytes, gx, stage, err, errlen, [] { return hipSuccess; }, [&](unsigned gx, const char* dtext) {
        hipLaunchKernelGGL(k_pat_count, dim3(gx), dim3(WG_BLOCK), 0, p->feed.st, dtext, n_bytes, p->start, p->end,
                           p->meth.as<int32_t>(), p->cov.as<int32_t>(), p->bad.as<unsigned long long>(), p->feed.fed);
    });
}

extern "C" {

int wgbsseg_patbeta_create(int device, int64_t start_cpg, int64_t end_cpg, wgbsseg_patbeta** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    if (start_cpg < 1 || end_cpg <= start_cpg || end_cpg - start_cpg > 0x7fffffff) { set_err(err, errlen, "patbeta: bad CpG range [%lld, %lld)", (long long)start_cpg, (long long)end_cpg); return WGBSSEG_E_ARG; }
    std::unique_ptr<wgbsseg_patbeta> p(new (std::nothrow) wgbsseg_patbeta());      // (a failing call below frees what has been made)
    if (!p) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    const int rc = p->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    p->start = start_cpg; p->end = end_cpg;
    const size_t nb = (size_t)(end_cpg - start_cpg) * 4;
    HIP_TRY(p->meth.ensure(nb)); HIP_TRY(p->cov.ensure(nb)); HIP_TRY(p->bad.ensure(8));
    HIP_TRY(hipMemsetAsync(p->meth.p, 0, nb, p->feed.st));       // (the reference leaves its arrays uninitialised: stdin2beta.cpp:48-49)
    HIP_TRY(hipMemsetAsync(p->cov.p, 0, nb, p->feed.st));
    HIP_TRY(hipMemsetAsync(p->bad.p, 0xff, 8, p->feed.st));
    *out = p.release();
    return WGBSSEG_OK;
}

void wgbsseg_patbeta_destroy(wgbsseg_patbeta* p) { delete p; }

int wgbsseg_patbeta_feed(wgbsseg_patbeta* p, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_text(p, text, n_bytes, err, errlen);
}

int wgbsseg_patbeta_feed_bgzf(wgbsseg_patbeta* p, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    return PatFeed::feed_bgzf(p, bytes, n_bytes, consumed, err, errlen);
}

int wgbsseg_patbeta_finish(wgbsseg_patbeta* p, int32_t lbeta, void* out, char* err, size_t errlen)
{
    if (!p || !out) { set_err(err, errlen, "bad arguments to patbeta_finish"); return WGBSSEG_E_ARG; }
    const hipStream_t st = p->feed.st;
    HIP_TRY(hipSetDevice(p->feed.device));
    int rc = PatFeed::flush_carry(p, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    const int64_t n = p->end - p->start;
    const size_t ob = (size_t)n * (lbeta ? 4 : 2);
    HIP_TRY(p->outb.ensure(ob));
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, p->bad.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rc = p->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (pat_refused(PatRefusal::bad_line, bad, "failed calculating beta:", err, errlen)) return WGBSSEG_E_ARG;
    hipLaunchKernelGGL(k_pat_trim, dim3((unsigned)((n + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, st, p->meth.as<int32_t>(), p->cov.as<int32_t>(), n,
                       (int)lbeta, p->outb.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, p->outb.p, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return WGBSSEG_OK;
}

double wgbsseg_patbeta_kernel_ms(wgbsseg_patbeta* p)
{
    return p ? p->feed.kernel_ms() : -1.0;
}

double wgbsseg_patbeta_inflate_ms(wgbsseg_patbeta* p)
{
    return p ? p->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

}  // extern "C"

// `wgbstools homog` accumulator: (block, bin) read counts on one device; k_homog_count is timed.
struct wgbsseg_homog {
    static constexpr const char* name = "homog";
    PatFeed feed;
    int64_t n_blocks = 0, last_end = 0;
    int n_bins = 0, min_cpgs = 0, inclusive = 0;
    DevBuf bstart, bend, bpmax, range, counts, bad, desc;
    PrevRead prev;
    ~wgbsseg_homog() { feed.drain(); }
};

// a staged chunk of n_bytes / gx tiles: k_homog_count over it
template <class Stage>
static int pat_chunk(wgbsseg_homog* h, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    return PatFeed::one_launch(h, n_bytes, gx, stage, err, errlen, [&] { return h->prev.carry(h->feed.st); }, [&](unsigned gx, const char* dtext) {
        hipLaunchKernelGGL(k_homog_count, dim3(gx), dim3(WG_BLOCK), 0, h->feed.st, dtext, n_bytes,
                           h->bstart.as<int32_t>(), h->bend.as<int32_t>(), h->bpmax.as<int32_t>(), h->n_blocks, h->last_end,
                           h->range.as<float>(), h->n_bins, h->min_cpgs, h->inclusive, h->counts.as<int32_t>(),
                           h->bad.as<unsigned long long>(), h->desc.as<unsigned long long>(), h->prev.in(), h->prev.out(), h->feed.fed);
        h->prev.chunks += 1;                                      // (the slots swap for the next chunk)
    });
}

extern "C" {

// plan (homog_plan.h) -> the tables and the edges on the device, the counters cleared
int wgbsseg_homog_create(int device, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, const float* range, int32_t n_bins,
                         int32_t min_cpgs, int32_t inclusive, wgbsseg_homog** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    HomogPlan plan;
    std::string msg;
    int rc = plan_homog(start_cpg, end_cpg, n_blocks, range, n_bins, min_cpgs, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    std::unique_ptr<wgbsseg_homog> h(new (std::nothrow) wgbsseg_homog());      // (a failing call below frees what has been made)
    if (!h) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    rc = h->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    h->n_blocks = n_blocks; h->last_end = plan.last_end;
    h->n_bins = n_bins; h->min_cpgs = min_cpgs; h->inclusive = inclusive ? 1 : 0;
    const hipStream_t st = h->feed.st;
    const size_t nb4 = (size_t)n_blocks * 4, cb = (size_t)n_blocks * (size_t)n_bins * 4;
    HIP_TRY(h->bstart.ensure(nb4)); HIP_TRY(h->bend.ensure(nb4)); HIP_TRY(h->bpmax.ensure(nb4));
    HIP_TRY(h->range.ensure(sizeof(float) * (size_t)(n_bins + 1))); HIP_TRY(h->counts.ensure(cb));
    HIP_TRY(h->bad.ensure(8)); HIP_TRY(h->desc.ensure(8)); HIP_TRY(h->prev.slots.ensure(16));
    HIP_TRY(hipMemcpy(h->bstart.p, plan.s32.data(), nb4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->bend.p, plan.e32.data(), nb4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->bpmax.p, plan.pmax.data(), nb4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->range.p, range, sizeof(float) * (size_t)(n_bins + 1), hipMemcpyHostToDevice));
    HIP_TRY(h->prev.reset());
    HIP_TRY(hipMemsetAsync(h->counts.p, 0, cb, st));
    HIP_TRY(hipMemsetAsync(h->bad.p, 0xff, 8, st));
    HIP_TRY(hipMemsetAsync(h->desc.p, 0xff, 8, st));
    *out = h.release();
    return WGBSSEG_OK;
}

void wgbsseg_homog_destroy(wgbsseg_homog* h) { delete h; }

int wgbsseg_homog_feed(wgbsseg_homog* h, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_text(h, text, n_bytes, err, errlen);
}

int wgbsseg_homog_feed_bgzf(wgbsseg_homog* h, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    return PatFeed::feed_bgzf(h, bytes, n_bytes, consumed, err, errlen);
}

int wgbsseg_homog_finish(wgbsseg_homog* h, int32_t* counts, char* err, size_t errlen)
{
    if (!h || !counts) { set_err(err, errlen, "bad arguments to homog_finish"); return WGBSSEG_E_ARG; }
    const hipStream_t st = h->feed.st;
    HIP_TRY(hipSetDevice(h->feed.device));
    int rc = PatFeed::flush_carry(h, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    unsigned long long bad = 0, desc = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->bad.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&desc, h->desc.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rc = h->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (pat_refused(PatRefusal::bad_line, bad, "failed calculating homog:", err, errlen)) return WGBSSEG_E_ARG;
    if (pat_refused(PatRefusal::unsorted, desc, "failed calculating homog:", err, errlen)) return WGBSSEG_E_ARG;
    HIP_TRY(hipMemcpyAsync(counts, h->counts.p, (size_t)h->n_blocks * (size_t)h->n_bins * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return WGBSSEG_OK;
}

double wgbsseg_homog_kernel_ms(wgbsseg_homog* h)
{
    return h ? h->feed.kernel_ms() : -1.0;
}

double wgbsseg_homog_inflate_ms(wgbsseg_homog* h)
{
    return h ? h->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

int wgbsseg_debug_homog_bins(const float* range, int32_t n_bins, int32_t max_total, int8_t* out)
{
    if (!range || !out || n_bins < 1 || n_bins > WG_HOMOG_MAX_BINS || max_total < 0 || max_total > 65535) return WGBSSEG_E_ARG;
    char err[256];
    const size_t errlen = sizeof(err);
    const int64_t n = (int64_t)(max_total + 1) * (max_total + 2) / 2;
    DevBuf d_range, d_out;
    HIP_TRY(d_range.ensure(sizeof(float) * (size_t)(n_bins + 1)));
    HIP_TRY(d_out.ensure((size_t)n));
    HIP_TRY(hipMemcpy(d_range.p, range, sizeof(float) * (size_t)(n_bins + 1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_homog_bins, dim3((unsigned)((n + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, 0, d_range.as<float>(), (int)n_bins, (int)max_total, d_out.as<int8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n, hipMemcpyDeviceToHost));
    return WGBSSEG_OK;
}

int wgbsseg_debug_bimodal_terms(const uint32_t* a, const uint32_t* b, int64_t count, uint64_t* out)
{
    if (!a || !b || !out || count < 1 || count > (1ll << 28)) return WGBSSEG_E_ARG;
    char err[256];
    const size_t errlen = sizeof(err);
    DevBuf d_ab, d_out;
    HIP_TRY(d_ab.ensure(2 * sizeof(uint32_t) * (size_t)count));
    HIP_TRY(d_out.ensure(6 * sizeof(uint64_t) * (size_t)count));
    uint32_t* const ab = d_ab.as<uint32_t>();
    HIP_TRY(hipMemcpy(ab, a, sizeof(uint32_t) * (size_t)count, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ab + count, b, sizeof(uint32_t) * (size_t)count, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)std::min<int64_t>((count + WG_BLOCK - 1) / WG_BLOCK, 16384);
    hipLaunchKernelGGL(k_bim_debug_terms, dim3(blocks), dim3(WG_BLOCK), 0, 0, ab, ab + count, count, d_out.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, 6 * sizeof(uint64_t) * (size_t)count, hipMemcpyDeviceToHost));
    return WGBSSEG_OK;
}

}  // extern "C"

// `wgbstools frag_len` accumulator: the histogram of the selected reads' lengths on one device; k_frag_hist is timed.
struct wgbsseg_fraglen {
    static constexpr const char* name = "fraglen";
    PatFeed feed;
    FragPlan plan;
    DevBuf bstart, bpmax, hist, bad, desc;
    PrevRead prev;
    ~wgbsseg_fraglen() { feed.drain(); }
};

// a staged chunk of n_bytes / gx tiles: k_frag_hist over it, min(gx, plan.groups) workgroups walking the tiles
template <class Stage>
static int pat_chunk(wgbsseg_fraglen* h, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    return PatFeed::one_launch(h, n_bytes, gx, stage, err, errlen, [&] { return h->prev.carry(h->feed.st); }, [&](unsigned gx, const char* dtext) {
        const unsigned grid = std::min<unsigned>(gx, (unsigned)h->plan.groups);
        hipLaunchKernelGGL(k_frag_hist, dim3(grid), dim3(WG_BLOCK), 0, h->feed.st, dtext, n_bytes, (int64_t)gx,
                           h->bstart.as<int32_t>(), h->bpmax.as<int32_t>(), h->plan.n_blocks, h->plan.end_last, (int)h->plan.max_frag,
                           h->hist.as<unsigned long long>(), h->bad.as<unsigned long long>(), h->desc.as<unsigned long long>(), h->prev.in(), h->prev.out(), h->feed.fed);
        h->prev.chunks += 1;                                      // (the slots swap for the next chunk)
    });
}

extern "C" {

// plan (frag_plan.h) -> the two tables on the device, the histogram and the edges cleared
int wgbsseg_fraglen_create(int device, int32_t max_frag, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t groups,
                           wgbsseg_fraglen** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    FragPlan plan;
    std::string msg;
    int rc = plan_frag(start_cpg, end_cpg, n_blocks, max_frag, plan, msg);
    if (rc == WGBSSEG_OK) rc = plan_frag_groups(groups, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    std::unique_ptr<wgbsseg_fraglen> h(new (std::nothrow) wgbsseg_fraglen());      // (a failing call below frees what has been made)
    if (!h) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    rc = h->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    h->plan = std::move(plan);
    const hipStream_t st = h->feed.st;
    const size_t nb4 = std::max<size_t>((size_t)n_blocks, 1) * 4, hb = (size_t)max_frag * 8;
    HIP_TRY(h->bstart.ensure(nb4)); HIP_TRY(h->bpmax.ensure(nb4)); HIP_TRY(h->hist.ensure(hb));
    HIP_TRY(h->bad.ensure(8)); HIP_TRY(h->desc.ensure(8)); HIP_TRY(h->prev.slots.ensure(16));
    if (n_blocks) {
        HIP_TRY(hipMemcpy(h->bstart.p, h->plan.start.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->bpmax.p, h->plan.pmax.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(h->prev.reset());
    HIP_TRY(hipMemsetAsync(h->hist.p, 0, hb, st));
    HIP_TRY(hipMemsetAsync(h->bad.p, 0xff, 8, st));
    HIP_TRY(hipMemsetAsync(h->desc.p, 0xff, 8, st));
    *out = h.release();
    return WGBSSEG_OK;
}

void wgbsseg_fraglen_destroy(wgbsseg_fraglen* h) { delete h; }

int wgbsseg_fraglen_feed(wgbsseg_fraglen* h, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_text(h, text, n_bytes, err, errlen);
}

int wgbsseg_fraglen_feed_bgzf(wgbsseg_fraglen* h, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    return PatFeed::feed_bgzf(h, bytes, n_bytes, consumed, err, errlen);
}

// the carry, then a refused BGZF member before a malformed line before a descending read, then the histogram
int wgbsseg_fraglen_finish(wgbsseg_fraglen* h, int64_t* hist, char* err, size_t errlen)
{
    if (!h || !hist) { set_err(err, errlen, "bad arguments to fraglen_finish"); return WGBSSEG_E_ARG; }
    const hipStream_t st = h->feed.st;
    HIP_TRY(hipSetDevice(h->feed.device));
    int rc = PatFeed::flush_carry(h, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    unsigned long long bad = 0, desc = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->bad.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&desc, h->desc.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rc = h->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (bad != ~0ULL) {
        set_err(err, errlen, "failed calculating frag_len: invalid line at byte offset %llu of the input (too few columns, a site / count that is not a number, or an empty pattern)", bad);
        return WGBSSEG_E_ARG;
    }
    if (pat_refused(PatRefusal::unsorted, desc, "failed calculating frag_len:", err, errlen)) return WGBSSEG_E_ARG;
    HIP_TRY(hipMemcpyAsync(hist, h->hist.p, (size_t)h->plan.max_frag * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return WGBSSEG_OK;
}

double wgbsseg_fraglen_kernel_ms(wgbsseg_fraglen* h)
{
    return h ? h->feed.kernel_ms() : -1.0;
}

double wgbsseg_fraglen_inflate_ms(wgbsseg_fraglen* h)
{
    return h ? h->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

}  // extern "C"

// `wgbstools test_bimodal` accumulator on one device: the plan of the blocks (bimodal_plan.h), the read table of the live window (two
// copies: dropping moves the live rows from one to the other), and the per-block results.  A feed() first waits for the work of the
// previous chunk (the caller inflated this chunk meanwhile), retires the blocks that chunk completed, drops the reads no pending block
// can reach, and queues the parse of this chunk; the EM of the retired blocks runs while the caller inflates the next one.  Every
// launch is timed.
struct wgbsseg_bimodal {
    struct Table { DevBuf start, len, cnt, woff, words; };
    static constexpr const char* name = "bimodal";
    PatFeed feed;
    BimodalPlan plan;
    int strict = 0, min_len = 1;
    int64_t pending = 0;                          // plan.by_end[pending..] have not been retired
    DevBuf bs1, bs2, ids, meta, scr_off, scratch, res_f, res_i, state, tile_cnt, tile_base, pos;
    Table tab[2];
    int cur = 0;
    size_t cap_rows = 0, cap_words = 0;
    PinnedBuf host_state, host_meta, host_off;
    bool stop = false;                            // an input error was seen: nothing more is computed
    wg_bim_state* hs() const { return reinterpret_cast<wg_bim_state*>(host_state.p); }
    ~wgbsseg_bimodal() { feed.drain(); }
};

static int bim_sync_state(wgbsseg_bimodal* b, char* err, size_t errlen)
{
    HIP_TRY(hipMemcpyAsync(b->host_state.p, b->state.p, sizeof(wg_bim_state), hipMemcpyDeviceToHost, b->feed.st));
    HIP_TRY(hipStreamSynchronize(b->feed.st));
    b->feed.collect();
    const wg_bim_state* s = b->hs();
    if (s->bad != ~0ULL || s->neg != ~0ULL || s->desc != ~0ULL || s->em_cap) b->stop = true;
    return WGBSSEG_OK;
}

// both tables hold at least `rows` reads and `words` words; the live rows of the current one are kept (the stream is idle)
static int bim_reserve(wgbsseg_bimodal* b, size_t rows, size_t words, char* err, size_t errlen)
{
    if (rows <= b->cap_rows && words <= b->cap_words) return WGBSSEG_OK;
    const size_t nr = std::max(rows, 2 * b->cap_rows), nw = std::max(words, 2 * b->cap_words);
    const size_t R = (size_t)b->hs()->R, W = (size_t)b->hs()->W;
    for (int t = 0; t < 2; t++) {
        wgbsseg_bimodal::Table fresh;
        HIP_TRY(fresh.start.ensure(nr * 4)); HIP_TRY(fresh.len.ensure(nr * 4)); HIP_TRY(fresh.cnt.ensure(nr * 4));
        HIP_TRY(fresh.woff.ensure(nr * 8)); HIP_TRY(fresh.words.ensure(nw * 4));
        wgbsseg_bimodal::Table& old = b->tab[t];
        if (t == b->cur && R) {
            HIP_TRY(hipMemcpy(fresh.start.p, old.start.p, R * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(fresh.len.p, old.len.p, R * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(fresh.cnt.p, old.cnt.p, R * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(fresh.woff.p, old.woff.p, R * 8, hipMemcpyDeviceToDevice));
        }
        if (t == b->cur && W) HIP_TRY(hipMemcpy(fresh.words.p, old.words.p, W * 4, hipMemcpyDeviceToDevice));
        old = std::move(fresh);                                 // (the old table's buffers go here)
    }
    b->cap_rows = nr; b->cap_words = nw;
    return WGBSSEG_OK;
}

// the EM of by_end[pending .. p1): their rows and columns, scratch for the wide ones, then k_bim_em (queued, not waited for)
static int bim_retire(wgbsseg_bimodal* b, int64_t p1, char* err, size_t errlen)
{
    const int64_t n = p1 - b->pending;
    if (n <= 0 || b->stop) return WGBSSEG_OK;
    wgbsseg_bimodal::Table& T = b->tab[b->cur];
    const int32_t* ids = b->plan.by_end.data() + b->pending;
    HIP_TRY(hipMemcpyAsync(b->ids.as<int32_t>(), ids, (size_t)n * 4, hipMemcpyHostToDevice, b->feed.st));
    HIP_TRY(b->feed.span_begin());
    hipLaunchKernelGGL(k_bim_gather, dim3((unsigned)n), dim3(WG_BIM_WAVE), 0, b->feed.st, T.start.as<int32_t>(), T.len.as<int32_t>(), T.cnt.as<int32_t>(),
                       b->state.as<wg_bim_state>(), b->bs1.as<int32_t>(), b->bs2.as<int32_t>(), b->ids.as<int32_t>(), b->strict, b->min_len,
                       b->meta.as<wg_bim_meta>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(b->feed.span_end());
    if (!b->host_meta.ensure((size_t)n * sizeof(wg_bim_meta))) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpyAsync(b->host_meta.p, b->meta.p, (size_t)n * sizeof(wg_bim_meta), hipMemcpyDeviceToHost, b->feed.st));
    HIP_TRY(hipStreamSynchronize(b->feed.st));
    if (!b->host_off.ensure((size_t)n * 8)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    long long* off = reinterpret_cast<long long*>(b->host_off.p);     // (read by the copy below after this returns: the next use waits for the stream)
    size_t used = 0;
    std::string msg;
    const int rc = wg_bim_scratch_layout(reinterpret_cast<const wg_bim_meta*>(b->host_meta.p), ids, n, b->plan.lds_cols, off, used, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (used) HIP_TRY(b->scratch.ensure(used));
    HIP_TRY(hipMemcpyAsync(b->scr_off.p, off, (size_t)n * 8, hipMemcpyHostToDevice, b->feed.st));
    HIP_TRY(b->feed.span_begin());
    hipLaunchKernelGGL(k_bim_em, dim3((unsigned)n), dim3(WG_BIM_WAVE), 0, b->feed.st, T.start.as<int32_t>(), T.len.as<int32_t>(), T.cnt.as<int32_t>(),
                       T.woff.as<long long>(), T.words.as<uint32_t>(), b->bs1.as<int32_t>(), b->bs2.as<int32_t>(), b->ids.as<int32_t>(),
                       b->meta.as<wg_bim_meta>(), b->scr_off.as<long long>(), b->scratch.as<unsigned char>(), b->plan.lds_cols, b->strict, b->min_len,
                       b->res_f.as<double>(), b->res_i.as<long long>(), b->state.as<wg_bim_state>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(b->feed.span_end());
    b->pending = p1;
    return WGBSSEG_OK;
}

// the reads no pending block can reach go: the live rows of the s.R reads / s.W words move into the other table, which becomes the current one
static int bim_drop(wgbsseg_bimodal* b, const wg_bim_state& s, char* err, size_t errlen)
{
    PatFeed& f = b->feed;
    wgbsseg_bimodal::Table &A = b->tab[b->cur], &B = b->tab[b->cur ^ 1];
    HIP_TRY(f.span_begin());
    hipLaunchKernelGGL(k_bim_drop_find, dim3(1), dim3(1), 0, f.st, A.start.as<int32_t>(), A.woff.as<long long>(), b->state.as<wg_bim_state>(),
                       b->plan.drop_below(b->pending));
    const long long big = std::max<long long>(s.R, s.W);
    hipLaunchKernelGGL(k_bim_drop_copy, dim3((unsigned)((big + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, f.st,
                       A.start.as<int32_t>(), A.len.as<int32_t>(), A.cnt.as<int32_t>(), A.woff.as<long long>(), A.words.as<uint32_t>(),
                       B.start.as<int32_t>(), B.len.as<int32_t>(), B.cnt.as<int32_t>(), B.woff.as<long long>(), B.words.as<uint32_t>(),
                       b->state.as<wg_bim_state>(), (long long)s.R, (long long)s.W);
    hipLaunchKernelGGL(k_bim_drop_done, dim3(1), dim3(1), 0, f.st, b->state.as<wg_bim_state>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(f.span_end());
    b->cur ^= 1;
    return WGBSSEG_OK;
}

// this chunk behind the table's reads: stage (the copy, either way), count, scan, fill, order (s: the state before it, ub: the bounds the tables were reserved for)
template <class Stage>
static int bim_parse_chunk(wgbsseg_bimodal* b, const wg_bim_state& s, Stage&& stage, int64_t n_bytes, int64_t gx, const BimodalChunkBound& ub,
                           char* err, size_t errlen)
{
    PatFeed& f = b->feed;
    HIP_TRY(b->tile_cnt.ensure((size_t)gx * 8)); HIP_TRY(b->tile_base.ensure((size_t)gx * 16)); HIP_TRY(b->pos.ensure(ub.lines * 8));
    const char* dtext = nullptr;
    const int rc = stage(&dtext);
    if (rc != WGBSSEG_OK) return rc;
    wgbsseg_bimodal::Table& T = b->tab[b->cur];
    HIP_TRY(f.span_begin());
    hipLaunchKernelGGL(k_bim_tile_count, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, b->tile_cnt.as<uint32_t>(),
                       b->state.as<wg_bim_state>(), f.fed);
    hipLaunchKernelGGL(k_bim_tile_scan, dim3(1), dim3(WG_BLOCK), 0, f.st, b->tile_cnt.as<uint32_t>(), gx, b->tile_base.as<long long>(),
                       b->state.as<wg_bim_state>());
    hipLaunchKernelGGL(k_bim_fill, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, b->tile_base.as<long long>(),
                       T.start.as<int32_t>(), T.len.as<int32_t>(), T.cnt.as<int32_t>(), T.woff.as<long long>(), T.words.as<uint32_t>(),
                       b->pos.as<long long>(), b->state.as<wg_bim_state>(), f.fed);
    hipLaunchKernelGGL(k_bim_order, dim3((unsigned)((ub.lines + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, f.st, T.start.as<int32_t>(),
                       b->pos.as<long long>(), b->state.as<wg_bim_state>(), s.last_start, (int64_t)ub.lines);
    HIP_TRY(hipGetLastError());
    HIP_TRY(f.span_end());
    HIP_TRY(f.chunk_queued(n_bytes));
    return WGBSSEG_OK;
}

// a chunk of n_bytes / gx tiles that stage() puts on the device:
// sync (the previous chunk is parsed and checked) -> reserve -> retire -> drop -> parse; every host decision is the plan's
template <class Stage>
static int pat_chunk(wgbsseg_bimodal* b, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    HIP_TRY(hipSetDevice(b->feed.device));
    int rc = bim_sync_state(b, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (b->stop) { b->feed.fed += (unsigned long long)n_bytes; return WGBSSEG_OK; }     // finish() reports the error
    const wg_bim_state s = *b->hs();
    const BimodalChunkBound ub(n_bytes);
    rc = bim_reserve(b, (size_t)s.R + ub.lines, (size_t)s.W + ub.words, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = bim_retire(b, b->plan.retire_upto(b->pending, s.last_start), err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (s.R > 0) rc = bim_drop(b, s, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    return bim_parse_chunk(b, s, stage, n_bytes, gx, ub, err, errlen);
}

extern "C" {

// plan (bimodal_plan.h) -> the blocks and a fresh state on the device
int wgbsseg_bimodal_create(int device, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t strict, int32_t min_len,
                           int32_t max_lds_cols, wgbsseg_bimodal** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    BimodalPlan plan;
    std::string msg;
    int rc = plan_bimodal(start_cpg, end_cpg, n_blocks, min_len, max_lds_cols, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    std::unique_ptr<wgbsseg_bimodal> b(new (std::nothrow) wgbsseg_bimodal());      // (a failing call below frees what has been made)
    if (!b) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    rc = b->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    b->plan = std::move(plan); b->strict = strict ? 1 : 0; b->min_len = min_len;
    const size_t nb = (size_t)n_blocks;
    HIP_TRY(b->bs1.ensure(nb * 4)); HIP_TRY(b->bs2.ensure(nb * 4)); HIP_TRY(b->ids.ensure(nb * 4));
    HIP_TRY(b->meta.ensure(nb * sizeof(wg_bim_meta))); HIP_TRY(b->scr_off.ensure(nb * 8));
    HIP_TRY(b->res_f.ensure(nb * 24)); HIP_TRY(b->res_i.ensure(nb * 24)); HIP_TRY(b->state.ensure(sizeof(wg_bim_state)));
    HIP_TRY(hipMemcpy(b->bs1.p, b->plan.s1.data(), nb * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->bs2.p, b->plan.s2.data(), nb * 4, hipMemcpyHostToDevice));
    if (!b->host_state.ensure(sizeof(wg_bim_state))) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    wg_bim_state s0;
    s0.R = s0.W = s0.R0 = 0; s0.last_start = WG_BIM_NONE; s0.head = s0.whead = 0;
    s0.bad = s0.neg = s0.desc = ~0ULL; s0.em_cap = 0;
    *b->hs() = s0;
    HIP_TRY(hipMemcpy(b->state.p, &s0, sizeof(s0), hipMemcpyHostToDevice));
    *out = b.release();
    return WGBSSEG_OK;
}

void wgbsseg_bimodal_destroy(wgbsseg_bimodal* b) { delete b; }

int wgbsseg_bimodal_feed(wgbsseg_bimodal* b, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_text(b, text, n_bytes, err, errlen);
}

int wgbsseg_bimodal_feed_bgzf(wgbsseg_bimodal* b, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    return PatFeed::feed_bgzf(b, bytes, n_bytes, consumed, err, errlen);
}

int wgbsseg_bimodal_finish(wgbsseg_bimodal* b, double* ll, int64_t* counts, char* err, size_t errlen)
{
    if (!b || !ll || !counts) { set_err(err, errlen, "bad arguments to bimodal_finish"); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(b->feed.device));
    int rc = PatFeed::flush_carry(b, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = bim_sync_state(b, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (!b->stop) {
        rc = bim_retire(b, b->plan.n_blocks, err, errlen);        // every read has been seen
        if (rc != WGBSSEG_OK) return rc;
        rc = bim_sync_state(b, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
    }
    rc = b->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    const wg_bim_state* s = b->hs();
    if (pat_refused(PatRefusal::bad_line, s->bad, "test_bimodal:", err, errlen)) return WGBSSEG_E_ARG;
    if (s->neg != ~0ULL) {
        set_err(err, errlen, "test_bimodal: negative read count at byte offset %llu of the input", s->neg);
        return WGBSSEG_E_ARG;
    }
    if (pat_refused(PatRefusal::unsorted, s->desc, "test_bimodal:", err, errlen)) return WGBSSEG_E_ARG;
    if (s->em_cap) {
        set_err(err, errlen, "test_bimodal: the EM of block %llu (row of the blocks) did not settle within %d iterations", s->em_cap, WG_BIM_MAX_ITERS);
        return WGBSSEG_E_CAPACITY;
    }
    HIP_TRY(hipMemcpy(ll, b->res_f.p, (size_t)b->plan.n_blocks * 24, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, b->res_i.p, (size_t)b->plan.n_blocks * 24, hipMemcpyDeviceToHost));
    return WGBSSEG_OK;
}

double wgbsseg_bimodal_kernel_ms(wgbsseg_bimodal* b)
{
    return b ? b->feed.kernel_ms() : -1.0;
}

double wgbsseg_bimodal_inflate_ms(wgbsseg_bimodal* b)
{
    return b ? b->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

// BGZF bytes -> the text of their complete members, inflated by k_bgzf_inflate (no line rule: every member goes to the device)
int wgbsseg_bgzf_inflate(int device, const void* bytes, int64_t n_bytes, void* out, int64_t out_cap, int64_t* out_len, int64_t* consumed, char* err, size_t errlen)
{
    if (!out_len || !consumed || n_bytes < 0 || out_cap < 0 || (n_bytes && !bytes) || (out_cap && !out)) { set_err(err, errlen, "bad arguments to bgzf_inflate"); return WGBSSEG_E_ARG; }
    *out_len = *consumed = 0;
    int rc = check_device(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    std::vector<wg_bgzf_member> members;
    std::string msg;
    int64_t used = 0;
    rc = bgzf_walk(static_cast<const uint8_t*>(bytes), n_bytes, 0, members, &used, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    const int64_t n_text = members.empty() ? 0 : (int64_t)(members.back().out_off + members.back().isize);
    if (n_text > out_cap) { set_err(err, errlen, "bgzf_inflate: %lld bytes of text, room for %lld", (long long)n_text, (long long)out_cap); return WGBSSEG_E_CAPACITY; }
    *consumed = used;
    if (members.empty()) return WGBSSEG_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t tb = members.size() * sizeof(wg_bgzf_member);
    DevBuf comp, text, bad;
    HIP_TRY(comp.ensure(tb + (size_t)used)); HIP_TRY(text.ensure((size_t)n_text + 1)); HIP_TRY(bad.ensure(8));
    HIP_TRY(hipMemcpy(comp.p, members.data(), tb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(comp.as<uint8_t>() + tb, bytes, (size_t)used, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(bad.p, 0xff, 8));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)((members.size() + WG_INF_WAVES - 1) / WG_INF_WAVES)), dim3(64 * WG_INF_WAVES), 0, 0,
                       comp.as<uint8_t>() + tb, comp.as<wg_bgzf_member>(), (int64_t)members.size(), text.as<uint8_t>(), bad.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long first_bad = ~0ULL;
    HIP_TRY(hipMemcpy(&first_bad, bad.p, 8, hipMemcpyDeviceToHost));
    if (n_text) HIP_TRY(hipMemcpy(out, text.p, (size_t)n_text, hipMemcpyDeviceToHost));
    *out_len = n_text;
    if (first_bad != ~0ULL) {
        (void)wg_inflate_refuse(msg, first_bad >> 8, (int)(first_bad & 0xff));
        set_err(err, errlen, "%s", msg.c_str());
        return WGBSSEG_E_ARG;
    }
    return WGBSSEG_OK;
}

}  // extern "C"

// `wgbstools view` / `cview` on one device: the surviving reads of every chunk as records + arena bytes (view_kernels.h), kept until
// finish(), which sorts (when asked), collapses and writes the text — or its BGZF form — on the device; read() fetches it in slabs.
// A chunk first waits for the chunk before it (the caller inflated this one meanwhile) and takes its totals, so the two buffers are
// sized by what they hold plus what this chunk can add (view_plan.h).  The chunk launches are the LAUNCHES span; the phases of finish()
// have events of their own.
struct wg_view_state {                                            // what the view's kernels leave on the device for the host (they take a pointer to each field)
    unsigned long long bad, desc;                                 // input offset of the first malformed line | of the first descending read; ~0: none
    uint32_t unsorted, too_big;                                   // k_view_inorder: a record lies before the one in front | k_view_runs: a count of 10^15 or more
    unsigned long long low;                                       // input offset of the first count below 1; ~0: none
};
static_assert(sizeof(wg_view_state) == 32 && offsetof(wg_view_state, desc) == 8 && offsetof(wg_view_state, unsorted) == 16 && offsetof(wg_view_state, too_big) == 20 && offsetof(wg_view_state, low) == 24, "the offsets the kernels' pointers were taken at");

struct wg_view_sample_state {                                     // with a source: what k_view_measure_sampled leaves
    unsigned long long over;                                      // input offset of the first line with count * reps above the cap; ~0: none
    unsigned long long stats[3];                                  // reads that reached the sampler, reads it dropped, the sum of the counts it kept
};

struct wgbsseg_patview {
    enum { SORT = 0, EMIT = 1, DEFLATE = 2 };
    static constexpr const char* name = "patview";
    PatFeed feed;
    ViewPlan plan;
    DevBuf recs, arena, tiles, totals, state;
    wg_view_state* dev_state() const { return state.as<wg_view_state>(); }
    PrevRead prev;
    ViewFiles files;                                              // the boundaries next_file() has recorded (view_plan.h)
    MaskPlan mask;                                                // set_mask(): the union of the hidden blocks (mask_plan.h) ...
    DevBuf mask_words, mask_iv;                                   // ... its bitmap on the device, and the intervals it was filled from
    bool masked = false, fed_any = false;                         // set_mask() has been called; feed() / feed_bgzf() has been called
    Event mask_ev[2];                                             // around k_view_mask_fill
    double mask_ms = 0.0;
    int64_t bgzf_left = 0;                                        // bytes the last feed_bgzf did not take
    ViewLabels labels;                                            // set_labels(): ranks and the table by rank (view_plan.h) ...
    DevBuf label_tab, sample;                                     // ... its offsets and bytes on the device | wg_view_sample_state
    bool labelled = false, file_fed = false;                      // set_labels() has been called; the open file has been fed
    int64_t source_file = -1;                                     // the file set_source() was last called for
    wg_view_source source = {};                                   // what it said (at / over / stats: filled per chunk)
    DevBuf perm[2], head, wg, run_end, run_tail, run_sum, tie_sum, tie_tail, text, slots, meta, dense;
    PinnedBuf host_tot, fetch;
    int64_t cap_recs = 0, cap_arena = 0;                          // what recs / arena have room for
    int64_t n_recs = 0, n_arena = 0;                              // what they hold (the chunks whose totals have been taken)
    bool pending = false;                                         // a chunk's totals are on their way to host_tot
    int64_t grown_recs = 0, grown_arena = 0;
    int passes = 0, order = 0;                                    // order: 0 no sort asked, 1 found in order, 2 sorted
    bool finished = false;
    const void* out = nullptr;                                    // the result on the device (text or dense) and its bytes
    int64_t out_bytes = 0;
    SamPlan sam_plan;                                             // set_sam(): the engine takes SAM text (sam_plan.h) ...
    bool sam = false;
    DevBuf sam_loci, sam_chroms;                                  // ... the loci and the chromosome table on the device
    DevBuf sam_tiles, sam_lines, sam_reads, sam_part, sam_head, sam_rid, sam_runs, sam_res, sam_wg;      // a chunk's tables (sam_kernels.h)
    DevBuf sam_carry, sam_state;                                  // two wg_sam_carry slots, swapped like PrevRead's | the counters, shift0
    PinnedBuf sam_home;                                           // the two totals a chunk sends home
    unsigned long long sam_chunks = 0;
    int64_t sam_lines_seen = 0;
    wg_sam_carry* sam_carry_in() const { return sam_carry.as<wg_sam_carry>() + ((sam_chunks & 1) ^ 1); }
    wg_sam_carry* sam_carry_out() const { return sam_carry.as<wg_sam_carry>() + (sam_chunks & 1); }
    unsigned long long* sam_counters() const { return sam_state.as<unsigned long long>(); }
    uint32_t* sam_shift0() const { return reinterpret_cast<uint32_t*>(sam_counters() + WG_SAM_COUNTERS); }
    Event ph[3][2];
    bool timed[3] = {false, false, false};
    double phase_ms[3] = {0.0, 0.0, 0.0};
    wg_view_args args() const { return {plan.s, plan.e, plan.min_len, plan.flags & (WG_VIEW_STRICT | WG_VIEW_STRIP | WG_VIEW_NO_GAPS)}; }
    wg_view_mask hidden() const { return {mask_words.as<const uint32_t>(), mask.lo, mask.hi}; }
    wg_view_labels label_table() const { return {label_tab.as<const char>() + (labels.n() + 1) * 4, label_tab.as<const uint32_t>()}; }
    wg_view_sample_state* dev_sample() const { return sample.as<wg_view_sample_state>(); }
    bool sampled() const { return labelled; }                    // with labels every file has a source (pat_chunk refuses a file without)
    ~wgbsseg_patview() { feed.drain(); }
};

// waits for the chunk before; its survivors and their bytes join the totals
static int view_take_totals(wgbsseg_patview* v, char* err, size_t errlen)
{
    HIP_TRY(hipStreamSynchronize(v->feed.st));
    v->feed.collect();
    if (v->pending) {
        const uint64_t* t = reinterpret_cast<const uint64_t*>(v->host_tot.p);
        v->n_recs += (int64_t)t[0]; v->n_arena += (int64_t)t[1];
        v->pending = false;
    }
    return WGBSSEG_OK;
}

// room for `recs` records and `bytes` arena bytes, by view_plan.h's growth rule; what the buffers hold is kept (the stream is idle)
static int view_reserve(wgbsseg_patview* v, int64_t recs, int64_t bytes, char* err, size_t errlen)
{
    const int64_t nr = wg_view_grow(v->cap_recs, recs), nb = wg_view_grow(v->cap_arena, bytes);
    if (nr != v->cap_recs) {
        DevBuf fresh;
        HIP_TRY(fresh.ensure((size_t)nr * sizeof(wg_view_rec)));
        if (v->n_recs) HIP_TRY(hipMemcpy(fresh.p, v->recs.p, (size_t)v->n_recs * sizeof(wg_view_rec), hipMemcpyDeviceToDevice));
        if (v->cap_recs) v->grown_recs++;
        v->recs = std::move(fresh);
        v->cap_recs = nr;
    }
    if (nb != v->cap_arena) {
        DevBuf fresh;
        HIP_TRY(fresh.ensure((size_t)nb));
        if (v->n_arena) HIP_TRY(hipMemcpy(fresh.p, v->arena.p, (size_t)v->n_arena, hipMemcpyDeviceToDevice));
        if (v->cap_arena) v->grown_arena++;
        v->arena = std::move(fresh);
        v->cap_arena = nb;
    }
    return WGBSSEG_OK;
}

// with labels every file needs a source before anything of it is fed
static int view_source_missing(const wgbsseg_patview* v, char* err, size_t errlen)
{
    if (!v->labelled || v->source_file == v->files.open_file()) return WGBSSEG_OK;
    set_err(err, errlen, "patview_feed: labels are set and file %lld has no source (patview_set_source)", (long long)v->files.open_file());
    return WGBSSEG_E_STATE;
}

// A staged chunk of SAM text (set_sam(); sam_kernels.h has the launch sequence): count the lines -> L comes home -> the per-line kernels
// up to the measure -> the records and arena bytes the chunk adds come home -> reserve -> pack.  Two waits per chunk: a pat cannot be
// bounded by the bytes of its line (D and N operations give sites without text), so the room is made from what was measured.
template <class Stage>
static int sam_chunk(wgbsseg_patview* v, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    PatFeed& f = v->feed;
    const hipStream_t st = f.st;
    std::string msg;
    SamChunk c;
    int rc = plan_sam_lines(n_bytes, 0, c, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    HIP_TRY(v->sam_tiles.ensure((size_t)(2 * gx + 2) * 8));
    const char* dtext = nullptr;
    rc = stage(&dtext);
    if (rc != WGBSSEG_OK) return rc;
    uint64_t *tile_lines = v->sam_tiles.as<uint64_t>(), *tile_base = tile_lines + gx, *ltot = tile_base + gx;
    uint64_t* home = static_cast<uint64_t*>(v->sam_home.p);
    HIP_TRY(hipMemcpyAsync(v->sam_carry_out(), v->sam_carry_in(), sizeof(wg_sam_carry), hipMemcpyDeviceToDevice, st));      // kept when the chunk holds no mate-able line
    HIP_TRY(f.span_begin());
    hipLaunchKernelGGL(k_sam_count, dim3((unsigned)gx), dim3(WG_BLOCK), 0, st, dtext, n_bytes, tile_lines);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, tile_lines, tile_lines, gx, tile_base, ltot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(f.span_end());
    HIP_TRY(hipMemcpyAsync(home, ltot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    f.collect();
    rc = plan_sam_lines(n_bytes, (int64_t)home[0], c, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (c.lines) {
        const size_t L = (size_t)c.lines;
        const int64_t G = c.groups;
        HIP_TRY(v->sam_lines.ensure(L * 4)); HIP_TRY(v->sam_reads.ensure(L * sizeof(wg_sam_read))); HIP_TRY(v->sam_part.ensure(L * 4));
        HIP_TRY(v->sam_head.ensure(L)); HIP_TRY(v->sam_rid.ensure(L * 4)); HIP_TRY(v->sam_runs.ensure(L * 4)); HIP_TRY(v->sam_res.ensure(L * sizeof(wg_sam_res)));
        HIP_TRY(v->sam_wg.ensure((size_t)c.wg_words() * 8));
        uint64_t *wg_part = v->sam_wg.as<uint64_t>(), *part_base = wg_part + G, *wg_heads = part_base + G, *head_base = wg_heads + G;
        uint64_t *wg_recs = head_base + G, *wg_bytes = wg_recs + G, *rec_base = wg_bytes + G, *byte_base = rec_base + G, *tot = byte_base + G;
        const wg_sam_args a = {dtext, n_bytes, v->sam_plan.chroms.view_at(v->sam_chroms.as<const char>()), v->sam_loci.as<const uint32_t>(), v->sam_plan.par};
        const dim3 grid((unsigned)G), block(WG_BLOCK), one(1);
        uint32_t *lstart = v->sam_lines.as<uint32_t>(), *part = v->sam_part.as<uint32_t>(), *rid = v->sam_rid.as<uint32_t>(), *runs = v->sam_runs.as<uint32_t>();
        wg_sam_read* reads = v->sam_reads.as<wg_sam_read>();
        wg_sam_res* res = v->sam_res.as<wg_sam_res>();
        HIP_TRY(f.span_begin());
        hipLaunchKernelGGL(k_sam_starts, dim3((unsigned)gx), block, 0, st, dtext, n_bytes, tile_base, lstart);
        hipLaunchKernelGGL(k_sam_eval, grid, block, 0, st, a, lstart, c.lines, reads, wg_part, v->sam_counters());
        hipLaunchKernelGGL(k_bed_scan, one, dim3(WG_BED_BLOCK), 0, st, wg_part, wg_part, G, part_base, tot);
        hipLaunchKernelGGL(k_sam_compact, grid, block, 0, st, reads, c.lines, part_base, part);
        hipLaunchKernelGGL(k_sam_heads, grid, block, 0, st, a, reads, part, tot, v->sam_carry_in(), v->sam_head.as<uint8_t>(), wg_heads, v->sam_shift0());
        hipLaunchKernelGGL(k_bed_scan, one, dim3(WG_BED_BLOCK), 0, st, wg_heads, wg_heads, G, head_base, tot + 2);
        hipLaunchKernelGGL(k_sam_runs, grid, block, 0, st, v->sam_head.as<const uint8_t>(), head_base, tot, rid, runs);
        hipLaunchKernelGGL(k_sam_measure, grid, block, 0, st, a, reads, part, tot, rid, runs, v->sam_shift0(), v->sam_carry_in(), v->recs.as<const wg_view_rec>(),
                           v->arena.as<const char>(), res, wg_recs, wg_bytes, v->sam_counters());
        hipLaunchKernelGGL(k_bed_scan, one, dim3(WG_BED_BLOCK), 0, st, wg_recs, wg_bytes, G, rec_base, tot + 4);      // tot[4], tot[5]: the records, the arena bytes
        hipLaunchKernelGGL(k_bed_scan, one, dim3(WG_BED_BLOCK), 0, st, wg_bytes, wg_bytes, G, byte_base, tot + 6);
        HIP_TRY(hipGetLastError());
        HIP_TRY(f.span_end());
        HIP_TRY(hipMemcpyAsync(home, tot + 4, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        f.collect();
        const int64_t added = (int64_t)home[0], bytes = (int64_t)home[1];
        rc = plan_sam_records(v->n_recs, added, msg);
        if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
        rc = view_reserve(v, v->n_recs + added, v->n_arena + bytes, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        HIP_TRY(f.span_begin());
        hipLaunchKernelGGL(k_sam_pack, grid, block, 0, st, a, reads, part, tot, rid, runs, v->sam_shift0(), v->sam_carry_in(), v->sam_carry_out(), res, rec_base, byte_base,
                           (uint64_t)v->n_recs, (uint64_t)v->n_arena, v->recs.as<wg_view_rec>(), v->arena.as<char>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(f.span_end());
        v->n_recs += added; v->n_arena += bytes;
        v->sam_lines_seen += c.lines;
    }
    v->sam_chunks += 1;                                            // (the carry's slots swap for the next chunk)
    HIP_TRY(f.chunk_queued(n_bytes));
    return WGBSSEG_OK;
}

// a staged chunk of n_bytes / gx tiles: totals of the chunk before -> reserve -> measure, scan, scan, pack -> its totals on their way
template <class Stage>
static int pat_chunk(wgbsseg_patview* v, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    PatFeed& f = v->feed;
    HIP_TRY(hipSetDevice(f.device));
    if (v->finished) { set_err(err, errlen, "patview_feed: finish() has been called"); return WGBSSEG_E_STATE; }
    if (v->sam) return sam_chunk(v, n_bytes, gx, stage, err, errlen);
    int rc = view_source_missing(v, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = view_take_totals(v, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    std::string msg;
    rc = plan_view_chunk(v->n_recs, n_bytes, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    rc = view_reserve(v, v->n_recs + wg_view_chunk_records(n_bytes), v->n_arena + n_bytes, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(v->tiles.ensure((size_t)gx * 32));
    const char* dtext = nullptr;
    rc = stage(&dtext);
    if (rc != WGBSSEG_OK) return rc;
    uint64_t *tile_recs = v->tiles.as<uint64_t>(), *tile_bytes = tile_recs + gx, *rec_base = tile_bytes + gx, *arena_base = rec_base + gx;
    uint64_t* tot = v->totals.as<uint64_t>();
    HIP_TRY(v->prev.carry(f.st));
    HIP_TRY(f.span_begin());
    wg_view_state* s = v->dev_state();
    wg_view_source q = v->source;
    if (v->sampled()) {                                            // the chunk's first byte inside its file; where the sampler reports
        q.at = f.fed - (v->files.several() ? (uint64_t)v->files.end_bytes.back() : 0u);
        q.over = &v->dev_sample()->over; q.stats = v->dev_sample()->stats;
    }
    if (v->sampled())
        hipLaunchKernelGGL(k_view_measure_sampled, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), q, tile_recs, tile_bytes,
                           &s->bad, &s->desc, &s->low, v->prev.in(), v->prev.out(), f.fed);
    else if (v->masked)
        hipLaunchKernelGGL(k_view_measure_masked, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), v->hidden(), tile_recs, tile_bytes,
                           &s->bad, &s->desc, &s->low, v->prev.in(), v->prev.out(), f.fed);
    else
        hipLaunchKernelGGL(k_view_measure, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), tile_recs, tile_bytes,
                           &s->bad, &s->desc, &s->low, v->prev.in(), v->prev.out(), f.fed);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, f.st, tile_recs, tile_bytes, gx, rec_base, tot);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, f.st, tile_bytes, tile_bytes, gx, arena_base, tot + 2);
    if (v->sampled())
        hipLaunchKernelGGL(k_view_pack_sampled, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), q, rec_base, arena_base,
                           (uint64_t)v->n_recs, (uint64_t)v->n_arena, v->recs.as<wg_view_rec>(), v->arena.as<char>());
    else if (v->masked)
        hipLaunchKernelGGL(k_view_pack_masked, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), v->hidden(), rec_base, arena_base,
                           (uint64_t)v->n_recs, (uint64_t)v->n_arena, v->recs.as<wg_view_rec>(), v->arena.as<char>());
    else
        hipLaunchKernelGGL(k_view_pack, dim3((unsigned)gx), dim3(WG_BLOCK), 0, f.st, dtext, n_bytes, v->args(), rec_base, arena_base,
                           (uint64_t)v->n_recs, (uint64_t)v->n_arena, v->recs.as<wg_view_rec>(), v->arena.as<char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(f.span_end());
    HIP_TRY(hipMemcpyAsync(v->host_tot.p, tot, 16, hipMemcpyDeviceToHost, f.st));
    v->pending = true;
    v->prev.chunks += 1;                                          // (the slots swap for the next chunk)
    HIP_TRY(f.chunk_queued(n_bytes));
    return WGBSSEG_OK;
}

static hipError_t view_phase(wgbsseg_patview* v, int which, int end)
{
    if (!end) v->timed[which] = true;
    return hipEventRecord(v->ph[which][end], v->feed.st);
}

// the permutation of the n records in sorted order -> *perm (nullptr: the input order is the sorted one)
static int view_sort(wgbsseg_patview* v, int64_t n, const uint32_t** perm, char* err, size_t errlen)
{
    const hipStream_t st = v->feed.st;
    const wg_view_rec* recs = v->recs.as<wg_view_rec>();
    const char* arena = v->arena.as<char>();
    uint32_t* unsorted = &v->dev_state()->unsorted;
    *perm = nullptr;
    HIP_TRY(view_phase(v, wgbsseg_patview::SORT, 0));
    const bool lab = v->labelled;                                  // the label rank as the last key: the _labelled instantiations
    hipLaunchKernelGGL(lab ? k_view_inorder_labelled : k_view_inorder, dim3((unsigned)((n + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, st, recs, arena, n, unsorted);
    HIP_TRY(hipGetLastError());
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, unsorted, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    v->order = flag ? 2 : 1;
    if (flag) {
        HIP_TRY(v->perm[0].ensure((size_t)n * 4)); HIP_TRY(v->perm[1].ensure((size_t)n * 4));
        int cur = 0;
        hipLaunchKernelGGL(lab ? k_view_sort_runs_labelled : k_view_sort_runs, dim3((unsigned)wg_view_runs(n)), dim3(WG_BLOCK), 0, st, recs, arena, n, v->perm[0].as<uint32_t>());
        const int passes = wg_view_merge_passes(n);
        int64_t run = WG_VIEW_RUN;
        const int64_t threads = (n + WG_VIEW_MERGE_ITEMS - 1) / WG_VIEW_MERGE_ITEMS;
        for (int k = 0; k < passes; k++, run *= 2, cur ^= 1)
            hipLaunchKernelGGL(lab ? k_view_merge_labelled : k_view_merge, dim3((unsigned)((threads + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, st, recs, arena, n, run,
                               v->perm[cur].as<const uint32_t>(), v->perm[cur ^ 1].as<uint32_t>());
        HIP_TRY(hipGetLastError());
        v->passes = passes;
        *perm = v->perm[cur].as<const uint32_t>();
    }
    HIP_TRY(view_phase(v, wgbsseg_patview::SORT, 1));
    return WGBSSEG_OK;
}

// the n records through `perm` -> the collapsed text in v->text; *lines, *bytes
static int view_emit(wgbsseg_patview* v, int64_t n, const uint32_t* perm, int64_t* lines, int64_t* bytes, char* err, size_t errlen)
{
    const hipStream_t st = v->feed.st;
    const wg_view_rec* recs = v->recs.as<wg_view_rec>();
    const char* arena = v->arena.as<char>();
    const int64_t nb = (n + WG_BLOCK - 1) / WG_BLOCK;
    HIP_TRY(v->head.ensure((size_t)n)); HIP_TRY(v->wg.ensure((size_t)(7 * nb + 6) * 8));
    HIP_TRY(v->run_end.ensure((size_t)n * 8)); HIP_TRY(v->run_tail.ensure((size_t)n * 4)); HIP_TRY(v->run_sum.ensure((size_t)n * 8));
    uint64_t *wg_counts = v->wg.as<uint64_t>(), *wg_heads = wg_counts + nb, *count_base = wg_heads + nb, *head_base = count_base + nb;
    uint64_t *wg_bytes = head_base + nb, *wg_lines = wg_bytes + nb, *line_base = wg_lines + nb, *tot = line_base + nb;      // tot: 3 pairs
    uint32_t* too_big = &v->dev_state()->too_big;
    const dim3 grid((unsigned)nb), block(WG_BLOCK);
    HIP_TRY(view_phase(v, wgbsseg_patview::EMIT, 0));
    hipLaunchKernelGGL(v->labelled ? k_view_heads_labelled : k_view_heads, grid, block, 0, st, recs, arena, perm, n, v->head.as<uint8_t>(), wg_counts, wg_heads);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, wg_counts, wg_heads, nb, count_base, tot);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, wg_heads, wg_heads, nb, head_base, tot + 2);
    hipLaunchKernelGGL(k_view_tails, grid, block, 0, st, recs, perm, n, v->head.as<const uint8_t>(), count_base, head_base, v->run_end.as<int64_t>(), v->run_tail.as<uint32_t>());
    const int64_t* sums = v->run_sum.as<const int64_t>();
    const uint32_t* tails = v->run_tail.as<const uint32_t>();
    if (v->labelled) {                                             // the runs of a group of tied lines into the reference's order, then the lengths with the labels
        HIP_TRY(v->tie_sum.ensure((size_t)n * 8)); HIP_TRY(v->tie_tail.ensure((size_t)n * 4));
        hipLaunchKernelGGL(k_view_run_sums, grid, block, 0, st, tot + 2, v->run_end.as<const int64_t>(), v->run_sum.as<int64_t>(), too_big);
        hipLaunchKernelGGL(k_view_tie_order, grid, block, 0, st, recs, arena, perm, tot + 2, sums, tails, v->tie_sum.as<int64_t>(), v->tie_tail.as<uint32_t>());
        sums = v->tie_sum.as<const int64_t>(); tails = v->tie_tail.as<const uint32_t>();
        hipLaunchKernelGGL(k_view_runs_labelled, grid, block, 0, st, recs, perm, tot + 2, sums, tails, v->label_table(), wg_bytes, wg_lines);
    } else
        hipLaunchKernelGGL(k_view_runs, grid, block, 0, st, recs, perm, tot + 2, v->run_end.as<const int64_t>(), v->run_tail.as<const uint32_t>(), v->run_sum.as<int64_t>(),
                           wg_bytes, wg_lines, too_big);
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, wg_bytes, wg_lines, nb, line_base, tot + 4);
    HIP_TRY(hipGetLastError());
    uint64_t got[2] = {0, 0};
    uint32_t big = 0;
    HIP_TRY(hipMemcpyAsync(got, tot + 4, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&big, too_big, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (big) {
        set_err(err, errlen, "failed in view: a collapsed count of 10^15 or more (the reference's collapse script would print it in exponent form)");
        return WGBSSEG_E_ARG;
    }
    HIP_TRY(v->text.ensure((size_t)got[0] + 16));
    if (v->labelled)
        hipLaunchKernelGGL(k_view_emit_labelled, grid, block, 0, st, recs, arena, perm, tot + 2, sums, tails, v->label_table(), line_base, v->text.as<char>());
    else
        hipLaunchKernelGGL(k_view_emit, grid, block, 0, st, recs, arena, perm, tot + 2, v->run_sum.as<const int64_t>(), v->run_tail.as<const uint32_t>(), line_base, v->text.as<char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(view_phase(v, wgbsseg_patview::EMIT, 1));
    *bytes = (int64_t)got[0]; *lines = (int64_t)got[1];
    return WGBSSEG_OK;
}

// v->text[0, n) -> BGZF members in v->dense, the end-of-file member behind them (the member rule and the kernels of wgbsseg_bgzf_deflate)
static int view_deflate(wgbsseg_patview* v, int64_t n, int64_t* bytes, char* err, size_t errlen)
{
    const hipStream_t st = v->feed.st;
    const int64_t members = wg_deflate_members(n), bound = wg_deflate_bound(n);
    if ((members + WG_DEF_WAVES - 1) / WG_DEF_WAVES > 0x7fffffff) { set_err(err, errlen, "view: too much text to deflate in one call"); return WGBSSEG_E_ARG; }
    HIP_TRY(v->dense.ensure((size_t)bound));
    uint64_t total = 0;
    if (members) {
        HIP_TRY(v->slots.ensure((size_t)members * WG_DEF_PITCH)); HIP_TRY(v->meta.ensure((size_t)(2 * members + 2) * 8));
        uint64_t *sizes = v->meta.as<uint64_t>(), *first = sizes + members, *dtot = first + members;
        HIP_TRY(view_phase(v, wgbsseg_patview::DEFLATE, 0));
        hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)((members + WG_DEF_WAVES - 1) / WG_DEF_WAVES)), dim3(64 * WG_DEF_WAVES), 0, st,
                           v->text.as<const uint8_t>(), n, members, v->slots.as<uint8_t>(), sizes);
        hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, sizes, sizes, members, first, dtot);
        hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)members), dim3(WG_PACK_BLOCK), 0, st, v->slots.as<const uint8_t>(), sizes, first, v->dense.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(view_phase(v, wgbsseg_patview::DEFLATE, 1));
        HIP_TRY(hipMemcpyAsync(&total, dtot, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)total > bound - (int64_t)sizeof(WG_BGZF_EOF)) { set_err(err, errlen, "view: %llu bytes came out of the deflate, more than the bound", (unsigned long long)total); return WGBSSEG_E_HIP; }
    }
    HIP_TRY(hipMemcpyAsync(v->dense.as<uint8_t>() + total, WG_BGZF_EOF, sizeof(WG_BGZF_EOF), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    *bytes = (int64_t)total + (int64_t)sizeof(WG_BGZF_EOF);
    return WGBSSEG_OK;
}

extern "C" {

int wgbsseg_patview_create(int device, int64_t start_cpg, int64_t end_cpg, int32_t flags, int32_t min_len, int64_t initial_records,
                           wgbsseg_patview** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    ViewPlan plan;
    std::string msg;
    int rc = plan_view(start_cpg, end_cpg, flags, min_len, initial_records, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    std::unique_ptr<wgbsseg_patview> v(new (std::nothrow) wgbsseg_patview());      // (a failing call below frees what has been made)
    if (!v) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    rc = v->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    v->plan = plan;
    for (auto& p : v->ph) for (auto& e : p) HIP_TRY(e.create());
    HIP_TRY(v->totals.ensure(32)); HIP_TRY(v->state.ensure(sizeof(wg_view_state))); HIP_TRY(v->prev.slots.ensure(16));
    if (!v->host_tot.ensure(16)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    rc = view_reserve(v.get(), plan.initial_records, plan.initial_records * 16, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(v->prev.reset());
    HIP_TRY(hipMemsetAsync(&v->dev_state()->bad, 0xff, offsetof(wg_view_state, unsorted), v->feed.st));        // bad, desc: none
    HIP_TRY(hipMemsetAsync(&v->dev_state()->unsorted, 0, offsetof(wg_view_state, low) - offsetof(wg_view_state, unsorted), v->feed.st));
    HIP_TRY(hipMemsetAsync(&v->dev_state()->low, 0xff, sizeof(wg_view_state::low), v->feed.st));
    *out = v.release();
    return WGBSSEG_OK;
}

void wgbsseg_patview_destroy(wgbsseg_patview* v) { delete v; }

// The site mask of `wgbstools mask_pat`: plan (mask_plan.h) -> the intervals to the device -> k_view_mask_fill on the feed's stream, in
// front of the first chunk's kernels.  Once, before anything has been fed: every read is cut by the same rule.
int wgbsseg_patview_set_mask(wgbsseg_patview* v, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, char* err, size_t errlen)
{
    if (!v) { set_err(err, errlen, "bad arguments to patview_set_mask"); return WGBSSEG_E_ARG; }
    if (v->masked) { set_err(err, errlen, "patview_set_mask: called twice"); return WGBSSEG_E_STATE; }
    if (v->fed_any || v->finished) { set_err(err, errlen, "patview_set_mask: called after the first feed"); return WGBSSEG_E_STATE; }
    if (v->sam) { set_err(err, errlen, "patview_set_mask: the engine takes SAM text: a mask does not go with it"); return WGBSSEG_E_STATE; }
    if (v->labelled) { set_err(err, errlen, "patview_set_mask: the engine has labels: a mask and sources do not go together"); return WGBSSEG_E_STATE; }
    MaskPlan plan;
    std::string msg;
    const int rc = plan_mask(start_cpg, end_cpg, n_blocks, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    const hipStream_t st = v->feed.st;
    HIP_TRY(hipSetDevice(v->feed.device));
    const size_t nk = (size_t)plan.n_intervals();
    HIP_TRY(v->mask_iv.ensure(2 * nk * 8)); HIP_TRY(v->mask_words.ensure((size_t)plan.n_words * 4));
    int64_t *starts = v->mask_iv.as<int64_t>(), *ends = starts + nk;
    HIP_TRY(hipMemcpyAsync(starts, plan.starts.data(), nk * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ends, plan.ends.data(), nk * 8, hipMemcpyHostToDevice, st));
    for (auto& e : v->mask_ev) HIP_TRY(e.create());
    HIP_TRY(hipEventRecord(v->mask_ev[0], st));
    hipLaunchKernelGGL(k_view_mask_fill, dim3((unsigned)((plan.n_words + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, st, starts, ends, (int64_t)nk, plan.lo,
                       plan.n_words, v->mask_words.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(v->mask_ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));                             // (the host vectors of the plan are pageable: the copies have left them)
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, v->mask_ev[0], v->mask_ev[1]) == hipSuccess) v->mask_ms = (double)ms;
    v->mask = std::move(plan);
    v->masked = true;
    return WGBSSEG_OK;
}

void wgbsseg_patview_mask_info(const wgbsseg_patview* v, int64_t* out)
{
    if (!v || !out) return;
    out[0] = v->mask.n_hidden; out[1] = v->mask.n_words; out[2] = v->masked ? 1 : 0;
}

double wgbsseg_patview_mask_ms(const wgbsseg_patview* v) { return v ? v->mask_ms : -1.0; }

// The labels of `wgbstools mix_pat`: plan (view_plan.h: the checks, the ranks) -> the table by rank to the device, once; the sampler's
// state beside it.  Once, before anything has been fed; from here on every file needs a source.
int wgbsseg_patview_set_labels(wgbsseg_patview* v, const char* const* labels, int64_t n, char* err, size_t errlen)
{
    if (!v) { set_err(err, errlen, "bad arguments to patview_set_labels"); return WGBSSEG_E_ARG; }
    if (v->labelled) { set_err(err, errlen, "patview_set_labels: called twice"); return WGBSSEG_E_STATE; }
    if (v->fed_any || v->finished) { set_err(err, errlen, "patview_set_labels: called after the first feed"); return WGBSSEG_E_STATE; }
    if (v->sam) { set_err(err, errlen, "patview_set_labels: the engine takes SAM text: labels do not go with it"); return WGBSSEG_E_STATE; }
    if (v->masked) { set_err(err, errlen, "patview_set_labels: the engine has a mask: a mask and sources do not go together"); return WGBSSEG_E_STATE; }
    ViewLabels plan;
    std::string msg;
    const int rc = plan_view_labels(labels, n, v->plan.flags, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    const hipStream_t st = v->feed.st;
    HIP_TRY(hipSetDevice(v->feed.device));
    const size_t ob = plan.off.size() * 4;
    HIP_TRY(v->label_tab.ensure(ob + plan.bytes.size())); HIP_TRY(v->sample.ensure(sizeof(wg_view_sample_state)));
    HIP_TRY(hipMemcpyAsync(v->label_tab.p, plan.off.data(), ob, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(v->label_tab.as<char>() + ob, plan.bytes.data(), plan.bytes.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(&v->dev_sample()->over, 0xff, sizeof(wg_view_sample_state::over), st));
    HIP_TRY(hipMemsetAsync(v->dev_sample()->stats, 0, sizeof(wg_view_sample_state::stats), st));
    HIP_TRY(hipStreamSynchronize(st));                             // (the plan's vectors are pageable: the copies have left them)
    v->labels = std::move(plan);
    v->labelled = true;
    return WGBSSEG_OK;
}

int32_t wgbsseg_patview_label_rank(const wgbsseg_patview* v, int64_t label)
{
    return v && label >= 0 && label < v->labels.n() ? (int32_t)v->labels.rank[(size_t)label] : -1;
}

// The source of the file about to be fed: host state only — the chunks of the file take it as a kernel argument.
int wgbsseg_patview_set_source(wgbsseg_patview* v, int32_t label_rank, uint32_t T, int32_t reps, uint64_t seed, uint32_t stream, char* err, size_t errlen)
{
    if (!v) { set_err(err, errlen, "bad arguments to patview_set_source"); return WGBSSEG_E_ARG; }
    if (v->finished) { set_err(err, errlen, "patview_set_source: finish() has been called"); return WGBSSEG_E_STATE; }
    if (v->file_fed) { set_err(err, errlen, "patview_set_source: file %lld has been fed already", (long long)v->files.open_file()); return WGBSSEG_E_STATE; }
    if (v->masked) { set_err(err, errlen, "patview_set_source: the engine has a mask: a mask and sources do not go together"); return WGBSSEG_E_STATE; }
    std::string msg;
    const int rc = plan_view_source(label_rank, T, reps, stream, v->labels.n(), msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    v->source = wg_view_source{seed, 0u, T, stream, (uint32_t)reps, (uint32_t)label_rank, nullptr, nullptr};
    v->source_file = v->files.open_file();
    return WGBSSEG_OK;
}

// SAM text in place of pat text (`wgbstools bam2pat`): plan (sam_plan.h: the checks, bed2beta_plan.h's chromosome table) -> the loci and
// the table to the device, the carry and the counters cleared.  Once, before anything has been fed.
int wgbsseg_patview_set_sam(wgbsseg_patview* v, const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo, const int64_t* chrom_hi,
                            int32_t n_chroms, int32_t paired, int64_t exclude_flags, int64_t include_flags, int32_t mapq, int32_t strand, int32_t clip, int32_t min_cpg,
                            char* err, size_t errlen)
{
    if (!v) { set_err(err, errlen, "bad arguments to patview_set_sam"); return WGBSSEG_E_ARG; }
    std::string msg;
    int rc = plan_sam_state(v->sam, v->fed_any, v->finished, v->masked, v->labelled, v->plan.flags, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    SamPlan plan;
    rc = plan_sam(loci, n_sites, chrom_names, chrom_lo, chrom_hi, n_chroms, paired, exclude_flags, include_flags, mapq, strand, clip, min_cpg, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    const hipStream_t st = v->feed.st;
    HIP_TRY(hipSetDevice(v->feed.device));
    std::vector<char> tab(plan.chroms.upload_bytes());
    plan.chroms.upload_to(tab.data());
    const size_t state_bytes = (WG_SAM_COUNTERS + 1) * 8;
    HIP_TRY(v->sam_loci.ensure((size_t)n_sites * 4)); HIP_TRY(v->sam_chroms.ensure(tab.size()));
    HIP_TRY(v->sam_carry.ensure(2 * sizeof(wg_sam_carry))); HIP_TRY(v->sam_state.ensure(state_bytes));
    if (!v->sam_home.ensure(16)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpy(v->sam_loci.p, loci, (size_t)n_sites * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->sam_chroms.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(v->sam_carry.p, 0, 2 * sizeof(wg_sam_carry), st));
    HIP_TRY(hipMemsetAsync(v->sam_state.p, 0, state_bytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    v->sam_plan = std::move(plan);
    v->sam = true;
    return WGBSSEG_OK;
}

void wgbsseg_patview_sam_info(wgbsseg_patview* v, int64_t* out)
{
    if (!v || !out) return;
    for (int k = 0; k < WG_SAM_COUNTERS; k++) out[k] = 0;
    if (!v->sam || hipSetDevice(v->feed.device) != hipSuccess || hipStreamSynchronize(v->feed.st) != hipSuccess) return;
    unsigned long long got[WG_SAM_COUNTERS];
    if (hipMemcpy(got, v->sam_counters(), sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int k = 0; k < WG_SAM_COUNTERS; k++) out[k] = (int64_t)got[k];
    out[WG_SAM_N_LINES] = v->sam_lines_seen;
}

void wgbsseg_patview_sample_info(wgbsseg_patview* v, int64_t* out)
{
    if (!v || !out) return;
    out[0] = out[1] = out[2] = 0;
    if (!v->labelled || hipSetDevice(v->feed.device) != hipSuccess || hipStreamSynchronize(v->feed.st) != hipSuccess) return;
    unsigned long long got[3] = {0, 0, 0};
    if (hipMemcpy(got, v->dev_sample()->stats, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int k = 0; k < 3; k++) out[k] = (int64_t)got[k];
}

int wgbsseg_patview_feed(wgbsseg_patview* v, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    if (v) {
        const int rc = view_source_missing(v, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        v->fed_any = v->file_fed = true;
    }
    return PatFeed::feed_text(v, text, n_bytes, err, errlen);
}

int wgbsseg_patview_feed_bgzf(wgbsseg_patview* v, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    if (v) {
        const int rc = view_source_missing(v, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        v->fed_any = v->file_fed = true;
    }
    const int rc = PatFeed::feed_bgzf(v, bytes, n_bytes, consumed, err, errlen);
    if (rc == WGBSSEG_OK) v->bgzf_left = n_bytes - *consumed;
    return rc;
}

// Between the feeds of two files: the carry (a last line without its newline) is fed as finish() feeds it; BGZF bytes left over are refused;
// the feed forgets the file — text or BGZF, the member offset, the read before — and the boundary goes into the host table.  What the
// files left in the record table and the arena stays: finish() sorts and collapses the records of all files, ties in input order.
int wgbsseg_patview_next_file(wgbsseg_patview* v, char* err, size_t errlen)
{
    if (!v) { set_err(err, errlen, "bad arguments to patview_next_file"); return WGBSSEG_E_ARG; }
    if (v->sam) { set_err(err, errlen, "patview_next_file: an engine that takes SAM text takes one file"); return WGBSSEG_E_STATE; }
    std::string msg;
    int rc = plan_view_next_file(v->finished, v->bgzf_left, v->files.open_file(), msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    PatFeed& f = v->feed;
    HIP_TRY(hipSetDevice(f.device));
    rc = PatFeed::flush_carry(v, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = view_take_totals(v, err, errlen);                         // (waits for the stream: the records of the file are counted)
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(v->prev.reset());                                      // the next file may begin below where this one ended
    f.mode = 0; f.file_off = 0; f.carry.clear();
    v->bgzf_left = 0;
    v->file_fed = false;
    v->files.close((int64_t)f.fed, v->n_recs);
    return WGBSSEG_OK;
}

// the carry; a refused BGZF member before a malformed line before a descending read; then sort, collapse, emit and (deflate) the BGZF form
int wgbsseg_patview_finish(wgbsseg_patview* v, int64_t* n_lines, int64_t* n_bytes, int32_t deflate, char* err, size_t errlen)
{
    if (!v || !n_lines || !n_bytes) { set_err(err, errlen, "bad arguments to patview_finish"); return WGBSSEG_E_ARG; }
    *n_lines = *n_bytes = 0;
    if (v->finished) { set_err(err, errlen, "patview_finish: called twice"); return WGBSSEG_E_STATE; }
    const hipStream_t st = v->feed.st;
    HIP_TRY(hipSetDevice(v->feed.device));
    int rc = PatFeed::flush_carry(v, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    v->finished = true;
    unsigned long long refused[2] = {0, 0}, low = 0, over = ~0ULL;
    if (v->labelled) HIP_TRY(hipMemcpyAsync(&over, &v->dev_sample()->over, sizeof(over), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(refused, &v->dev_state()->bad, sizeof(refused), hipMemcpyDeviceToHost, st));      // bad, desc
    HIP_TRY(hipMemcpyAsync(&low, &v->dev_state()->low, sizeof(low), hipMemcpyDeviceToHost, st));
    rc = view_take_totals(v, err, errlen);                         // (waits for the stream)
    if (rc != WGBSSEG_OK) return rc;
    rc = v->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (v->files.several()) {                                      // several files: the file and the offset inside it; a count below 1 is refused
        const ViewRefusal why[3] = {ViewRefusal::bad_line, ViewRefusal::unsorted, ViewRefusal::low_count};
        const unsigned long long at[3] = {refused[0], refused[1], low};
        for (int k = 0; k < 3; k++)
            if (at[k] != ~0ULL) { set_err(err, errlen, "%s", wg_view_file_refusal(v->files, why[k], at[k]).c_str()); return WGBSSEG_E_ARG; }
    }
    if (refused[0] != ~0ULL) {
        set_err(err, errlen, "failed in view: invalid line at byte offset %llu of the input (too few columns, a site / count that is not a number, an empty pattern, or something between the count and the end of the line)", refused[0]);
        return WGBSSEG_E_ARG;
    }
    if (pat_refused(PatRefusal::unsorted, refused[1], "failed in view:", err, errlen)) return WGBSSEG_E_ARG;
    if ((v->masked || v->labelled) && low != ~0ULL) {              // a mask, labels: a count below 1 is refused in a single file too (merge's reason)
        set_err(err, errlen, "failed in view: count < 1 at byte %llu", low);
        return WGBSSEG_E_ARG;
    }
    if (over != ~0ULL) { set_err(err, errlen, "%s", wg_view_over_refusal(v->files, over).c_str()); return WGBSSEG_E_ARG; }
    const int64_t n = v->n_recs;
    int64_t lines = 0, bytes = 0;
    if (n) {
        const uint32_t* perm = nullptr;
        if (v->plan.flags & WG_VIEW_SORT) {
            rc = view_sort(v, n, &perm, err, errlen);
            if (rc != WGBSSEG_OK) return rc;
        }
        rc = view_emit(v, n, perm, &lines, &bytes, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
    }
    v->out = v->text.p; v->out_bytes = bytes;
    if (deflate) {
        rc = view_deflate(v, bytes, &v->out_bytes, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        v->out = v->dense.p;
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 3; k++) {
        float ms = 0.f;
        if (v->timed[k] && hipEventElapsedTime(&ms, v->ph[k][0], v->ph[k][1]) == hipSuccess) v->phase_ms[k] = (double)ms;
    }
    *n_lines = lines; *n_bytes = v->out_bytes;
    return WGBSSEG_OK;
}

// bytes [offset, offset + len) of the result, in slabs through page-locked staging
int wgbsseg_patview_read(wgbsseg_patview* v, int64_t offset, void* buf, int64_t len, char* err, size_t errlen)
{
    if (!v || !v->finished) { set_err(err, errlen, "patview_read: nothing to read before finish()"); return WGBSSEG_E_STATE; }
    std::string msg;
    const int rc = plan_view_read(offset, len, v->out_bytes, buf, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (len == 0) return WGBSSEG_OK;
    HIP_TRY(hipSetDevice(v->feed.device));
    if (!v->fetch.ensure_exact((size_t)std::min<int64_t>(len, WG_VIEW_SLAB))) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    const char* src = static_cast<const char*>(v->out) + offset;
    for (int64_t k = 0; k < wg_view_slabs(len); k++) {
        const int64_t nb = wg_view_slab_len(len, k);
        HIP_TRY(hipMemcpyAsync(v->fetch.p, src + k * WG_VIEW_SLAB, (size_t)nb, hipMemcpyDeviceToHost, v->feed.st));
        HIP_TRY(hipStreamSynchronize(v->feed.st));
        memcpy(static_cast<char*>(buf) + k * WG_VIEW_SLAB, v->fetch.p, (size_t)nb);
    }
    return WGBSSEG_OK;
}

double wgbsseg_patview_kernel_ms(wgbsseg_patview* v)
{
    return v ? v->feed.kernel_ms() : -1.0;
}

double wgbsseg_patview_inflate_ms(wgbsseg_patview* v)
{
    return v ? v->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

void wgbsseg_patview_phase_ms(const wgbsseg_patview* v, double* sort_ms, double* emit_ms, double* deflate_ms)
{
    if (sort_ms) *sort_ms = v ? v->phase_ms[wgbsseg_patview::SORT] : 0.0;
    if (emit_ms) *emit_ms = v ? v->phase_ms[wgbsseg_patview::EMIT] : 0.0;
    if (deflate_ms) *deflate_ms = v ? v->phase_ms[wgbsseg_patview::DEFLATE] : 0.0;
}

void wgbsseg_patview_info(const wgbsseg_patview* v, int64_t* out)
{
    if (!v || !out) return;
    out[0] = v->n_recs; out[1] = v->n_arena; out[2] = v->grown_recs; out[3] = v->grown_arena; out[4] = v->passes; out[5] = v->order;
}

}  // extern "C"

// `wgbstools bed2beta` accumulator on one device: the loci and the chromosome table (bed2beta_plan.h) uploaded once, one 64-bit word per
// site that k_bedbeta_scan lowers to the first matching line of the file (timed), the report words; finish() unpacks the table into the
// .beta bytes, next_file() clears it for the next file.
struct wgbsseg_bedbeta {
    static constexpr const char* name = "bedbeta";
    PatFeed feed;
    BedBetaPlan plan;
    int32_t flags = 0;
    DevBuf loci, chroms, table, outb, report;
    int64_t bgzf_left = 0;                                        // bytes the last feed_bgzf did not take
    unsigned long long* dev_report() const { return report.as<unsigned long long>(); }
    ~wgbsseg_bedbeta() { feed.drain(); }
};

// the table all ones, the report: no refused line, the counters 0 (queued on the feed's stream)
static hipError_t bedbeta_clear(wgbsseg_bedbeta* b)
{
    hipError_t e = hipMemsetAsync(b->table.p, 0xff, (size_t)b->plan.n_words * 8, b->feed.st);
    if (e == hipSuccess) e = hipMemsetAsync(b->report.p, 0xff, 8, b->feed.st);
    if (e == hipSuccess) e = hipMemsetAsync(b->dev_report() + 1, 0, (WG_BB_REP_WORDS - 1) * 8, b->feed.st);
    return e;
}

// a staged chunk of n_bytes / gx tiles: k_bedbeta_scan over it
template <class Stage>
static int pat_chunk(wgbsseg_bedbeta* b, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    std::string msg;
    const int rc = plan_bedbeta_chunk(b->feed.fed, n_bytes, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    return PatFeed::one_launch(b, n_bytes, gx, stage, err, errlen, [] { return hipSuccess; }, [&](unsigned gx, const char* dtext) {
        hipLaunchKernelGGL(k_bedbeta_scan, dim3(gx), dim3(WG_BLOCK), 0, b->feed.st, dtext, n_bytes, b->plan.view_at(b->chroms.as<const char>()),
                           b->loci.as<const uint32_t>(), (b->flags & WG_BB_ADD_ONE) ? 1 : 0, (b->flags & WG_BB_HEADER) ? 1 : 0,
                           b->table.as<unsigned long long>(), b->dev_report(), b->feed.fed);
    });
}

extern "C" {

// plan (bed2beta_plan.h) -> the loci and the chromosome table on the device, the table and the report cleared
int wgbsseg_bedbeta_create(int device, const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo,
                           const int64_t* chrom_hi, int32_t n_chroms, int32_t flags, wgbsseg_bedbeta** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    BedBetaPlan plan;
    std::string msg;
    int rc = plan_bedbeta(loci, n_sites, chrom_names, chrom_lo, chrom_hi, n_chroms, flags, plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    std::unique_ptr<wgbsseg_bedbeta> b(new (std::nothrow) wgbsseg_bedbeta());      // (a failing call below frees what has been made)
    if (!b) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    rc = b->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    b->plan = std::move(plan);
    b->flags = flags;
    const BedBetaPlan& p = b->plan;
    std::vector<char> tab(p.upload_bytes());
    p.upload_to(tab.data());
    HIP_TRY(b->loci.ensure((size_t)n_sites * 4)); HIP_TRY(b->chroms.ensure(tab.size()));
    HIP_TRY(b->table.ensure((size_t)p.n_words * 8)); HIP_TRY(b->outb.ensure((size_t)p.n_words * 2)); HIP_TRY(b->report.ensure(WG_BB_REP_WORDS * 8));
    HIP_TRY(hipMemcpy(b->loci.p, loci, (size_t)n_sites * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->chroms.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(bedbeta_clear(b.get()));
    *out = b.release();
    return WGBSSEG_OK;
}

void wgbsseg_bedbeta_destroy(wgbsseg_bedbeta* b) { delete b; }

int wgbsseg_bedbeta_feed(wgbsseg_bedbeta* b, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_text(b, text, n_bytes, err, errlen);
}

int wgbsseg_bedbeta_feed_bgzf(wgbsseg_bedbeta* b, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    const int rc = PatFeed::feed_bgzf(b, bytes, n_bytes, consumed, err, errlen);
    if (rc == WGBSSEG_OK) b->bgzf_left = n_bytes - *consumed;
    return rc;
}

// the carry; a refused BGZF member before a refused line; then the table unpacked into the .beta bytes, and the counters
int wgbsseg_bedbeta_finish(wgbsseg_bedbeta* b, uint8_t* out, int64_t* stats, char* err, size_t errlen)
{
    if (!b || !out) { set_err(err, errlen, "bad arguments to bedbeta_finish"); return WGBSSEG_E_ARG; }
    const hipStream_t st = b->feed.st;
    HIP_TRY(hipSetDevice(b->feed.device));
    int rc = PatFeed::flush_carry(b, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    unsigned long long rep[WG_BB_REP_WORDS];
    HIP_TRY(hipMemcpyAsync(rep, b->report.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rc = b->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    std::string msg;
    if (wg_bb_refusal(rep[WG_BB_REP_BAD], msg)) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    const int64_t n_threads = b->plan.n_words / WG_BB_UNPACK_SITES;
    HIP_TRY(hipMemsetAsync(b->dev_report() + WG_BB_REP_SET, 0, 8, st));      // (finish() may be called again)
    hipLaunchKernelGGL(k_bedbeta_unpack, dim3((unsigned)((n_threads + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, st,
                       b->table.as<const unsigned long long>(), n_threads, b->outb.as<uint8_t>(), b->dev_report());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, b->outb.p, (size_t)b->plan.n_sites * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rep, b->report.p, sizeof(rep), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) {
        stats[0] = (int64_t)rep[WG_BB_REP_LINES]; stats[1] = (int64_t)rep[WG_BB_REP_MATCHED];
        stats[2] = (int64_t)rep[WG_BB_REP_NO_CHROM]; stats[3] = (int64_t)rep[WG_BB_REP_NO_CPG];
        stats[4] = (int64_t)(rep[WG_BB_REP_MATCHED] - rep[WG_BB_REP_SET]); stats[5] = (int64_t)rep[WG_BB_REP_SET];
    }
    return WGBSSEG_OK;
}

// Between two files: BGZF bytes left over are refused; the feed forgets the file — text or BGZF, the member offset, the carry, the bytes
// fed (offsets count from 0 again) —, the table, the report and the counters are cleared, and `flags` are the next file's.
int wgbsseg_bedbeta_next_file(wgbsseg_bedbeta* b, int32_t flags, char* err, size_t errlen)
{
    if (!b) { set_err(err, errlen, "bad arguments to bedbeta_next_file"); return WGBSSEG_E_ARG; }
    std::string msg;
    const int rc = plan_bedbeta_flags(flags, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (b->bgzf_left) { set_err(err, errlen, "bedbeta_next_file: %lld bytes behind the file's last whole BGZF member", (long long)b->bgzf_left); return WGBSSEG_E_ARG; }
    PatFeed& f = b->feed;
    HIP_TRY(hipSetDevice(f.device));
    HIP_TRY(bedbeta_clear(b));
    f.mode = 0; f.file_off = 0; f.fed = 0; f.carry.clear();
    b->bgzf_left = 0;
    b->flags = flags;
    return WGBSSEG_OK;
}

double wgbsseg_bedbeta_kernel_ms(wgbsseg_bedbeta* b)
{
    return b ? b->feed.kernel_ms() : -1.0;
}

double wgbsseg_bedbeta_inflate_ms(wgbsseg_bedbeta* b)
{
    return b ? b->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

}  // extern "C"

// `wgbstools init_genome` on one device: FASTA text through the feed's byte-cut path (a chunk may end anywhere) -> the sequence table and
// the loci of every CpG in FASTA order (fasta_kernels.h has the launch sequence; the carry between chunks is a few words on the device);
// then select() gathers the kept sequences' loci in dictionary order (that array is loci.u32) and dict() writes `name \t locus \t site`
// for them and deflates the text into BGZF by the codec's launch sequence.  The chunk launches are the LAUNCHES span; gather, emit and
// deflate have events of their own.
struct wgbsseg_fasta {
    enum { GATHER = 0, EMIT = 1, DEFLATE = 2 };
    static constexpr const char* name = "fasta";
    PatFeed feed;
    DevBuf tiles, entries, carry, bad, totals, seqs, loci;
    PinnedBuf home;
    int64_t cap_seqs = 0, cap_loci = 0;                           // what seqs / loci have room for
    int64_t n_seqs = 0, n_loci = 0;                               // what they hold (the chunks fed so far)
    bool scanned = false, selected = false, written = false;
    std::vector<wg_fa_seq> table;                                 // finish_scan(): the records at home ...
    std::vector<int64_t> n_bases, n_sites;                        // ... and what follows from them
    DevBuf sel, cum, names, name_len, wg, text, slots, meta, dense;
    int64_t n_sel = 0, n_chroms = 0;
    const void* out = nullptr;
    int64_t out_bytes = 0;
    PinnedBuf fetch;
    Event ph[3][2];
    bool timed[3] = {false, false, false};
    double phase_ms[3] = {0.0, 0.0, 0.0};
    ~wgbsseg_fasta() { feed.drain(); }
};

// room for `seqs` records and `loci` loci, by view_plan.h's growth rule; what the buffers hold is kept (the stream is idle)
static int fasta_reserve(wgbsseg_fasta* f, int64_t seqs, int64_t loci, char* err, size_t errlen)
{
    const int64_t ns = wg_view_grow(f->cap_seqs, seqs), nl = wg_view_grow(f->cap_loci, loci);
    if (ns != f->cap_seqs) {
        DevBuf fresh;
        HIP_TRY(fresh.ensure((size_t)ns * sizeof(wg_fa_seq)));
        if (f->n_seqs) HIP_TRY(hipMemcpy(fresh.p, f->seqs.p, (size_t)f->n_seqs * sizeof(wg_fa_seq), hipMemcpyDeviceToDevice));
        f->seqs = std::move(fresh);
        f->cap_seqs = ns;
    }
    if (nl != f->cap_loci) {
        DevBuf fresh;
        HIP_TRY(fresh.ensure((size_t)nl * 4));
        if (f->n_loci) HIP_TRY(hipMemcpy(fresh.p, f->loci.p, (size_t)f->n_loci * 4, hipMemcpyDeviceToDevice));
        f->loci = std::move(fresh);
        f->cap_loci = nl;
    }
    return WGBSSEG_OK;
}

static hipError_t fasta_phase(wgbsseg_fasta* f, int which, int end)
{
    if (!end) f->timed[which] = true;
    return hipEventRecord(f->ph[which][end], f->feed.st);
}

static void fasta_read_phases(wgbsseg_fasta* f)
{
    for (int k = 0; k < 3; k++) {
        float ms = 0.f;
        if (f->timed[k] && hipEventElapsedTime(&ms, f->ph[k][0], f->ph[k][1]) == hipSuccess) f->phase_ms[k] = (double)ms;
    }
}

// A staged chunk of n_bytes / gx tiles: settle the pending C -> measure -> scan -> the totals come home (the first wait) -> reserve ->
// pack.  The second wait is the staging slot's, two chunks on.  The loci buffer always has room for one site more than it holds: the
// next chunk's k_fa_settle may add the pending one.
template <class Stage>
static int pat_chunk(wgbsseg_fasta* f, int64_t n_bytes, int64_t gx, Stage&& stage, char* err, size_t errlen)
{
    PatFeed& fd = f->feed;
    const hipStream_t st = fd.st;
    HIP_TRY(hipSetDevice(fd.device));
    if (f->scanned) { set_err(err, errlen, "fasta_feed: finish_scan() has been called"); return WGBSSEG_E_STATE; }
    std::string msg;
    int rc = plan_fasta_chunk(n_bytes, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    HIP_TRY(f->tiles.ensure((size_t)gx * sizeof(wg_fa_tile))); HIP_TRY(f->entries.ensure((size_t)gx * sizeof(wg_fa_entry)));
    const char* dtext = nullptr;
    rc = stage(&dtext);
    if (rc != WGBSSEG_OK) return rc;
    wg_fa_carry* carry = f->carry.as<wg_fa_carry>();
    uint64_t* home = static_cast<uint64_t*>(f->home.p);
    HIP_TRY(fd.span_begin());
    hipLaunchKernelGGL(k_fa_settle, dim3(1), dim3(1), 0, st, dtext, n_bytes, carry, f->loci.as<uint32_t>());
    hipLaunchKernelGGL(k_fa_measure, dim3((unsigned)gx), dim3(WG_FA_BLOCK), 0, st, dtext, n_bytes, f->tiles.as<wg_fa_tile>());
    hipLaunchKernelGGL(k_fa_scan, dim3(1), dim3(WG_FA_SCAN_BLOCK), 0, st, f->tiles.as<const wg_fa_tile>(), gx, (uint64_t)fd.fed, carry, f->entries.as<wg_fa_entry>(),
                       f->totals.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(fd.span_end());
    HIP_TRY(hipMemcpyAsync(home, f->totals.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    fd.collect();
    const int64_t seqs = (int64_t)home[0], loci = (int64_t)home[1];
    if (seqs < f->n_seqs || loci < f->n_loci || seqs - f->n_seqs > n_bytes || loci - f->n_loci > n_bytes + 1) {
        set_err(err, errlen, "fasta: the scan of a chunk of %lld bytes reports %lld sequences and %lld sites behind %lld and %lld", (long long)n_bytes, (long long)seqs,
                (long long)loci, (long long)f->n_seqs, (long long)f->n_loci);
        return WGBSSEG_E_HIP;
    }
    rc = fasta_reserve(f, seqs, loci + 1, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    f->n_seqs = seqs; f->n_loci = loci;
    HIP_TRY(fd.span_begin());
    hipLaunchKernelGGL(k_fa_pack, dim3((unsigned)gx), dim3(WG_FA_BLOCK), 0, st, dtext, n_bytes, (uint64_t)fd.fed, f->entries.as<const wg_fa_entry>(), f->seqs.as<wg_fa_seq>(),
                       f->loci.as<uint32_t>(), f->bad.as<unsigned long long>(), carry);
    HIP_TRY(hipGetLastError());
    HIP_TRY(fd.span_end());
    HIP_TRY(fd.chunk_queued(n_bytes));
    return WGBSSEG_OK;
}

// text[0, n) deflated into f->dense, the end-of-file member behind it (the member rule and the kernels of wgbsseg_bgzf_deflate)
static int fasta_deflate(wgbsseg_fasta* f, int64_t n, int64_t* bytes, char* err, size_t errlen)
{
    const hipStream_t st = f->feed.st;
    const int64_t members = wg_deflate_members(n), bound = wg_deflate_bound(n);
    if ((members + WG_DEF_WAVES - 1) / WG_DEF_WAVES > 0x7fffffff) { set_err(err, errlen, "fasta_dict: too much text to deflate in one call"); return WGBSSEG_E_ARG; }
    HIP_TRY(f->dense.ensure((size_t)bound));
    uint64_t total = 0;
    if (members) {
        HIP_TRY(f->slots.ensure((size_t)members * WG_DEF_PITCH)); HIP_TRY(f->meta.ensure((size_t)(2 * members + 2) * 8));
        uint64_t *sizes = f->meta.as<uint64_t>(), *first = sizes + members, *dtot = first + members;
        HIP_TRY(fasta_phase(f, wgbsseg_fasta::DEFLATE, 0));
        hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)((members + WG_DEF_WAVES - 1) / WG_DEF_WAVES)), dim3(64 * WG_DEF_WAVES), 0, st,
                           f->text.as<const uint8_t>(), n, members, f->slots.as<uint8_t>(), sizes);
        hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, sizes, sizes, members, first, dtot);
        hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)members), dim3(WG_PACK_BLOCK), 0, st, f->slots.as<const uint8_t>(), sizes, first, f->dense.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(fasta_phase(f, wgbsseg_fasta::DEFLATE, 1));
        HIP_TRY(hipMemcpyAsync(&total, dtot, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)total > bound - (int64_t)sizeof(WG_BGZF_EOF)) { set_err(err, errlen, "fasta_dict: %llu bytes came out of the deflate, more than the bound", (unsigned long long)total); return WGBSSEG_E_HIP; }
    }
    HIP_TRY(hipMemcpyAsync(f->dense.as<uint8_t>() + total, WG_BGZF_EOF, sizeof(WG_BGZF_EOF), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    *bytes = (int64_t)total + (int64_t)sizeof(WG_BGZF_EOF);
    return WGBSSEG_OK;
}

// what wgbsseg_debug_fasta_walk's walk leaves: the tables of the caller
struct FastaHostSink {
    int64_t cap_seqs, cap_loci;
    int64_t *hdr_off, *prev_bases, *first_locus;
    int32_t* name_len;
    char* names;
    uint32_t* loci;
    uint64_t bad = ~0ULL;
    bool full = false;
    void header(const wg_fa_cur& c, uint64_t at)
    {
        if ((int64_t)c.seqs >= cap_seqs) { full = true; return; }
        hdr_off[c.seqs] = (int64_t)at; first_locus[c.seqs] = (int64_t)c.hits; prev_bases[c.seqs] = (int64_t)c.bases; name_len[c.seqs] = -1;
    }
    void name_byte(uint64_t seq, uint32_t idx, char b) { if ((int64_t)seq < cap_seqs) names[seq * (WG_FA_MAX_NAME + 1) + idx] = b; }
    void name_end(uint64_t seq, uint64_t len) { if ((int64_t)seq < cap_seqs) name_len[seq] = (int32_t)std::min<uint64_t>(len, WG_FA_MAX_NAME + 1); }
    void hit(uint64_t index, uint64_t locus) { if ((int64_t)index < cap_loci) loci[index] = (uint32_t)locus; else full = true; }
    void pending(uint64_t) {}                                      // (the text ends: no next base)
    void refuse(uint64_t at, int why) { bad = std::min<uint64_t>(bad, (at << 8) | (uint64_t)why); }
};

extern "C" {

int wgbsseg_fasta_create(int device, wgbsseg_fasta** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    std::unique_ptr<wgbsseg_fasta> f(new (std::nothrow) wgbsseg_fasta());      // (a failing call below frees what has been made)
    if (!f) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    int rc = f->feed.open(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    for (auto& p : f->ph) for (auto& e : p) HIP_TRY(e.create());
    HIP_TRY(f->carry.ensure(sizeof(wg_fa_carry))); HIP_TRY(f->bad.ensure(8)); HIP_TRY(f->totals.ensure(16));
    if (!f->home.ensure(16)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    rc = fasta_reserve(f.get(), WG_FA_INITIAL_SEQS, WG_FA_INITIAL_LOCI, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(hipMemsetAsync(f->carry.p, 0, sizeof(wg_fa_carry), f->feed.st));      // at the start of a line, nothing seen, nothing pending
    HIP_TRY(hipMemsetAsync(f->bad.p, 0xff, 8, f->feed.st));
    *out = f.release();
    return WGBSSEG_OK;
}

void wgbsseg_fasta_destroy(wgbsseg_fasta* f) { delete f; }

int wgbsseg_fasta_feed(wgbsseg_fasta* f, const char* text, int64_t n_bytes, char* err, size_t errlen)
{
    return PatFeed::feed_bytes(f, text, n_bytes, err, errlen);
}

int wgbsseg_fasta_feed_bgzf(wgbsseg_fasta* f, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen)
{
    return PatFeed::feed_bgzf_bytes(f, bytes, n_bytes, consumed, err, errlen);
}

// The end of the input: a refused BGZF member before a refusal of the text; the record table comes home, the last sequence is closed
// (a C left pending has no next base), two sequences of one name are refused.  counts: sequences, sites, bytes of text.
int wgbsseg_fasta_finish_scan(wgbsseg_fasta* f, int64_t* counts, char* err, size_t errlen)
{
    if (!f || !counts) { set_err(err, errlen, "bad arguments to fasta_finish_scan"); return WGBSSEG_E_ARG; }
    if (f->scanned) { set_err(err, errlen, "fasta_finish_scan: called twice"); return WGBSSEG_E_STATE; }
    const hipStream_t st = f->feed.st;
    HIP_TRY(hipSetDevice(f->feed.device));
    f->scanned = true;
    wg_fa_carry carry;
    unsigned long long bad = ~0ULL;
    HIP_TRY(hipMemcpyAsync(&carry, f->carry.p, sizeof(carry), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, f->bad.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    f->feed.collect();
    int rc = f->feed.inflate_refused(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    std::string msg;
    if (bad != ~0ULL) { rc = wg_fa_refuse(msg, bad); set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if ((int64_t)carry.seqs != f->n_seqs || (int64_t)carry.hits != f->n_loci) { set_err(err, errlen, "fasta_finish_scan: the carry and the totals disagree"); return WGBSSEG_E_HIP; }
    const size_t n = (size_t)f->n_seqs;
    f->table.resize(n);
    if (n) HIP_TRY(hipMemcpy(f->table.data(), f->seqs.p, n * sizeof(wg_fa_seq), hipMemcpyDeviceToHost));
    if (n && carry.state == WG_FA_NM) {                            // the text ends inside the last name
        const uint64_t len = (uint64_t)f->feed.fed - carry.hdr_off - 1;
        if (len == 0) { rc = wg_fa_refuse(msg, (carry.hdr_off << 8) | WG_FA_BAD_EMPTY_NAME); set_err(err, errlen, "%s", msg.c_str()); return rc; }
        f->table[n - 1].name_len = (uint32_t)len;
    }
    f->n_bases.assign(n, 0); f->n_sites.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        f->n_bases[i] = i + 1 < n ? (int64_t)f->table[i + 1].prev_bases : (int64_t)carry.bases;
        f->n_sites[i] = (int64_t)((i + 1 < n ? f->table[i + 1].first_locus : (uint64_t)f->n_loci) - f->table[i].first_locus);
    }
    rc = plan_fasta_names(f->table, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    counts[0] = f->n_seqs; counts[1] = f->n_loci; counts[2] = (int64_t)f->feed.fed;
    return WGBSSEG_OK;
}

// the table of finish_scan(): per sequence the offset of its header, its bases, its sites, the length of its name and the name
// (WG_FA_MAX_NAME + 1 bytes each, zero-padded)
int wgbsseg_fasta_sequences(wgbsseg_fasta* f, int64_t* hdr_off, int64_t* n_bases, int64_t* n_sites, int32_t* name_len, char* names, char* err, size_t errlen)
{
    if (!f || !f->scanned) { set_err(err, errlen, "fasta_sequences: nothing to read before finish_scan()"); return WGBSSEG_E_STATE; }
    for (size_t i = 0; i < f->table.size(); i++) {
        const wg_fa_seq& s = f->table[i];
        if (hdr_off) hdr_off[i] = (int64_t)s.hdr_off;
        if (n_bases) n_bases[i] = f->n_bases[i];
        if (n_sites) n_sites[i] = f->n_sites[i];
        if (name_len) name_len[i] = (int32_t)s.name_len;
        if (names) {
            char* dst = names + i * (WG_FA_MAX_NAME + 1);
            memset(dst, 0, WG_FA_MAX_NAME + 1);
            memcpy(dst, s.name, std::min<size_t>(s.name_len, WG_FA_MAX_NAME));
        }
    }
    return WGBSSEG_OK;
}

// The kept sequences in dictionary order: their loci gathered into one array (a device-to-device copy per sequence), the cumulative
// table and the names to the device.  *n_sites: the sites of the dictionary.
int wgbsseg_fasta_select(wgbsseg_fasta* f, const int64_t* order, int64_t n_order, int64_t* n_sites, char* err, size_t errlen)
{
    if (!f || !n_sites) { set_err(err, errlen, "bad arguments to fasta_select"); return WGBSSEG_E_ARG; }
    if (!f->scanned || f->table.size() != (size_t)f->n_seqs) { set_err(err, errlen, "fasta_select: finish_scan() comes first"); return WGBSSEG_E_STATE; }
    std::string msg;
    int64_t total = 0;
    const int rc = plan_fasta_select(order, n_order, f->n_seqs, f->n_sites, &total, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    const hipStream_t st = f->feed.st;
    HIP_TRY(hipSetDevice(f->feed.device));
    std::vector<int64_t> cum((size_t)n_order);
    std::vector<uint32_t> lens((size_t)n_order);
    std::vector<char> names((size_t)n_order * (WG_FA_MAX_NAME + 1), 0);
    HIP_TRY(f->sel.ensure((size_t)std::max<int64_t>(total, 1) * 4)); HIP_TRY(f->cum.ensure(cum.size() * 8)); HIP_TRY(f->name_len.ensure(lens.size() * 4));
    HIP_TRY(f->names.ensure(names.size()));
    HIP_TRY(fasta_phase(f, wgbsseg_fasta::GATHER, 0));
    int64_t at = 0;
    for (int64_t k = 0; k < n_order; k++) {
        const wg_fa_seq& s = f->table[(size_t)order[k]];
        const int64_t m = f->n_sites[(size_t)order[k]];
        if (m) HIP_TRY(hipMemcpyAsync(f->sel.as<uint32_t>() + at, f->loci.as<uint32_t>() + s.first_locus, (size_t)m * 4, hipMemcpyDeviceToDevice, st));
        at += m;
        cum[(size_t)k] = at; lens[(size_t)k] = s.name_len;
        memcpy(names.data() + (size_t)k * (WG_FA_MAX_NAME + 1), s.name, s.name_len);
    }
    HIP_TRY(fasta_phase(f, wgbsseg_fasta::GATHER, 1));
    HIP_TRY(hipMemcpyAsync(f->cum.p, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(f->name_len.p, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(f->names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                             // (the vectors go)
    fasta_read_phases(f);
    f->n_sel = total; f->n_chroms = n_order;
    f->selected = true; f->written = false;
    *n_sites = total;
    return WGBSSEG_OK;
}

// the gathered loci: what loci.u32 holds
int wgbsseg_fasta_loci(wgbsseg_fasta* f, uint32_t* out, int64_t n, char* err, size_t errlen)
{
    if (!f || !f->selected) { set_err(err, errlen, "fasta_loci: select() comes first"); return WGBSSEG_E_STATE; }
    if (n != f->n_sel || (n && !out)) { set_err(err, errlen, "fasta_loci: room for %lld loci, the dictionary has %lld", (long long)n, (long long)f->n_sel); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(f->feed.device));
    if (n) HIP_TRY(hipMemcpyAsync(out, f->sel.p, (size_t)n * 4, hipMemcpyDeviceToHost, f->feed.st));
    HIP_TRY(hipStreamSynchronize(f->feed.st));
    return WGBSSEG_OK;
}

// the dictionary's text (CpG.bed) for the selected sites, as BGZF with deflate; it stays on the device for read()
int wgbsseg_fasta_dict(wgbsseg_fasta* f, int32_t deflate, int64_t* n_lines, int64_t* n_bytes, char* err, size_t errlen)
{
    if (!f || !n_lines || !n_bytes) { set_err(err, errlen, "bad arguments to fasta_dict"); return WGBSSEG_E_ARG; }
    *n_lines = *n_bytes = 0;
    if (!f->selected) { set_err(err, errlen, "fasta_dict: select() comes first"); return WGBSSEG_E_STATE; }
    const hipStream_t st = f->feed.st;
    HIP_TRY(hipSetDevice(f->feed.device));
    const int64_t n = f->n_sel, nb = (n + WG_FA_DICT_BLOCK - 1) / WG_FA_DICT_BLOCK;
    uint64_t got[2] = {0, 0};
    if (n) {
        HIP_TRY(f->wg.ensure((size_t)(3 * nb + 2) * 8));
        uint64_t *wg_bytes = f->wg.as<uint64_t>(), *wg_lines = wg_bytes + nb, *wg_base = wg_lines + nb, *tot = wg_base + nb;
        const wg_dict_args a = {f->sel.as<const uint32_t>(), f->cum.as<const int64_t>(), f->names.as<const char>(), f->name_len.as<const uint32_t>(), n, (int32_t)f->n_chroms};
        HIP_TRY(fasta_phase(f, wgbsseg_fasta::EMIT, 0));
        hipLaunchKernelGGL(k_dict_len, dim3((unsigned)nb), dim3(WG_FA_DICT_BLOCK), 0, st, a, wg_bytes, wg_lines);
        hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, st, wg_bytes, wg_lines, nb, wg_base, tot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(got, tot, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)got[1] != n || got[0] > (uint64_t)n * WG_FA_DICT_MAX_LINE) { set_err(err, errlen, "fasta_dict: %llu bytes in %llu lines for %lld sites", (unsigned long long)got[0], (unsigned long long)got[1], (long long)n); return WGBSSEG_E_HIP; }
        HIP_TRY(f->text.ensure((size_t)got[0] + 16));
        hipLaunchKernelGGL(k_dict_emit, dim3((unsigned)nb), dim3(WG_FA_DICT_BLOCK), 0, st, a, wg_base, f->text.as<char>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(fasta_phase(f, wgbsseg_fasta::EMIT, 1));
    } else
        HIP_TRY(f->text.ensure(16));
    f->out = f->text.p; f->out_bytes = (int64_t)got[0];
    if (deflate) {
        const int rc = fasta_deflate(f, (int64_t)got[0], &f->out_bytes, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        f->out = f->dense.p;
    }
    HIP_TRY(hipStreamSynchronize(st));
    fasta_read_phases(f);
    f->written = true;
    *n_lines = n; *n_bytes = f->out_bytes;
    return WGBSSEG_OK;
}

// bytes [offset, offset + len) of dict()'s result, in slabs through page-locked staging
int wgbsseg_fasta_read(wgbsseg_fasta* f, int64_t offset, void* buf, int64_t len, char* err, size_t errlen)
{
    if (!f || !f->written) { set_err(err, errlen, "fasta_read: nothing to read before dict()"); return WGBSSEG_E_STATE; }
    std::string msg;
    const int rc = plan_view_read(offset, len, f->out_bytes, buf, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (len == 0) return WGBSSEG_OK;
    HIP_TRY(hipSetDevice(f->feed.device));
    if (!f->fetch.ensure_exact((size_t)std::min<int64_t>(len, WG_VIEW_SLAB))) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    const char* src = static_cast<const char*>(f->out) + offset;
    for (int64_t k = 0; k < wg_view_slabs(len); k++) {
        const int64_t nb = wg_view_slab_len(len, k);
        HIP_TRY(hipMemcpyAsync(f->fetch.p, src + k * WG_VIEW_SLAB, (size_t)nb, hipMemcpyDeviceToHost, f->feed.st));
        HIP_TRY(hipStreamSynchronize(f->feed.st));
        memcpy(static_cast<char*>(buf) + k * WG_VIEW_SLAB, f->fetch.p, (size_t)nb);
    }
    return WGBSSEG_OK;
}

double wgbsseg_fasta_kernel_ms(wgbsseg_fasta* f)
{
    return f ? f->feed.kernel_ms() : -1.0;
}

double wgbsseg_fasta_inflate_ms(wgbsseg_fasta* f)
{
    return f ? f->feed.kernel_ms(PatFeed::INFLATE) : -1.0;
}

void wgbsseg_fasta_phase_ms(const wgbsseg_fasta* f, double* gather_ms, double* emit_ms, double* deflate_ms)
{
    if (gather_ms) *gather_ms = f ? f->phase_ms[wgbsseg_fasta::GATHER] : 0.0;
    if (emit_ms) *emit_ms = f ? f->phase_ms[wgbsseg_fasta::EMIT] : 0.0;
    if (deflate_ms) *deflate_ms = f ? f->phase_ms[wgbsseg_fasta::DEFLATE] : 0.0;
}

// The rule on the host, serially: fasta_core.h's walk over text[0, n) — what the engine's kernels run 16 bytes at a time — into the
// caller's tables (room for cap_seqs sequences and cap_loci loci; names: WG_FA_MAX_NAME + 1 bytes per sequence).  counts: sequences,
// sites.  *refused: (offset << 8 | reason) of the first refusal, ~0: none.  No device is touched.
int wgbsseg_debug_fasta_walk(const char* text, int64_t n, int64_t cap_seqs, int64_t cap_loci, int64_t* hdr_off, int64_t* n_bases, int64_t* n_sites, int32_t* name_len,
                             char* names, uint32_t* loci, int64_t* counts, uint64_t* refused)
{
    if (n < 0 || (n && !text) || cap_seqs < 0 || cap_loci < 0 || !counts || !refused) return WGBSSEG_E_ARG;
    if (cap_seqs && (!hdr_off || !n_bases || !n_sites || !name_len || !names)) return WGBSSEG_E_ARG;
    if (cap_loci && !loci) return WGBSSEG_E_ARG;
    std::vector<int64_t> prev((size_t)cap_seqs), first((size_t)cap_seqs);
    if (cap_seqs) memset(names, 0, (size_t)cap_seqs * (WG_FA_MAX_NAME + 1));
    FastaHostSink k = {cap_seqs, cap_loci, hdr_off, prev.data(), first.data(), name_len, names, loci};
    wg_fa_cur c = {0, 0, 0, 0, WG_FA_LS};
    const wg_fa_plain_text T = {text};
    wg_fa_walk(T, n, 0, n, 0, c, k);
    counts[0] = (int64_t)c.seqs; counts[1] = (int64_t)c.hits;
    *refused = k.bad;
    if (k.full) return WGBSSEG_E_CAPACITY;
    const int64_t m = (int64_t)c.seqs;
    if (m && c.state == WG_FA_NM) {                                // the text ends inside the last name
        const uint64_t len = (uint64_t)n - c.hdr_off - 1;
        if (len == 0) *refused = std::min<uint64_t>(*refused, (c.hdr_off << 8) | WG_FA_BAD_EMPTY_NAME);
        name_len[m - 1] = (int32_t)std::min<uint64_t>(len, WG_FA_MAX_NAME + 1);
    }
    for (int64_t i = 0; i < m; i++) {
        n_bases[i] = i + 1 < m ? prev[(size_t)i + 1] : (int64_t)c.bases;
        n_sites[i] = (i + 1 < m ? first[(size_t)i + 1] : (int64_t)c.hits) - first[(size_t)i];
    }
    return WGBSSEG_OK;
}

}  // extern "C"
