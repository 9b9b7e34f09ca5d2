// gfx950 URI kernels of the logparser_amd engine (HttpUriDissector,
// QueryStringFieldDissector): k_uri_lines, its direct path k_uri_overflow,
// which also redoes the lines whose URI the reference repairs, and the
// derived (type-remapped) stages k_derived_lines.  They run after
// the parse kernels, one wave per 64 lines of the batch's line index.
#include "kernels_common.h"

namespace lp {

namespace {

// ------------------------------------------------------------------ URIs
// The URI and query-string stages of a wave's 64 lines (HttpUriDissector,
// QueryStringFieldDissector), after the parse kernels wrote the lines' status and
// spans.  Each lane's URI sources (request URI, referer, ...) are gathered
// from the input into a compact LDS buffer (only the URI bytes: a few KiB per
// wave, so many waves share a CU and hide the arena atomics and the query
// passes' latencies), with their one-plane UEV mask; then phase 2 per lane,
// a wave-aggregated arena allocation, and the query pieces spread over the
// lanes.  A wave whose URI bytes do not fit runs on the direct (HBM) path.
// compact URI bytes per wave: with its mask plane within the LDS share of a
// CU running 16 waves (config 2: 7.3 KiB per wave on average, 8.3 KiB at the
// 99th percentile; a wave needing more runs on the direct path)
constexpr uint32_t URI_CAP = 8512;
// query pieces per lane per round of the piece pass; gather rounds per batch
// (experiment builds override them: make exp XFLAGS=-DLP_URI_QR=...)
#ifndef LP_URI_QR
#define LP_URI_QR 4
#endif
#ifndef LP_URI_GR
#define LP_URI_GR 9
#endif

// Which lane's line owns item g0 + lane of a cooperative pass (the gather's
// blocks, the walk's events, the piece pass's pieces; lp_owner.h): the
// lanes' items numbered line after line, `first` = the exclusive prefix sum
// of the counts.  The kernel is bound by VALU issue more than by latency, so
// the lookup is kept to a few VALU instructions and two LDS reads: the
// owner's rank among the non-empty lanes from the round's head mask
// (owner_rank), then the rank table, which holds select64(N, r) and that
// lane's first item for every r (each non-empty lane writes its own entry,
// once per pass).  The head masks of OWNER_WORDS rounds at a time live in
// LDS: fill(b0) has every non-empty lane whose first item lies in
// [b0, b0 + 64 OWNER_WORDS) OR its bit into its round's word (workgroups are
// one wave: the barriers only order the LDS accesses).  All wave-uniform
// control flow; every lane takes part.
constexpr int OWNER_WORDS = LP_URI_GR;
constexpr int OWNER_LDS_WORDS = OWNER_WORDS + PW / 2;  // uint64_t: the head words, then PW 32-bit table entries
struct OwnerRounds {
    uint64_t* hw;
    uint32_t* tab;   // entry r: the r-th non-empty lane | its first item << 6
    uint32_t first;  // this lane's first item
    bool has;        // this lane has items
    uint32_t b0;     // the first item of the filled rounds

    __device__ __forceinline__ OwnerRounds(uint64_t* words, uint32_t first_item, uint32_t cnt)
        : hw(words), tab(reinterpret_cast<uint32_t*>(words + OWNER_WORDS)), first(first_item), has(cnt != 0), b0(0) {
        const uint64_t N = __ballot(has);
        const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(N >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)N, 0u));
        __syncthreads();  // the previous pass has read its table
        if (has) tab[r] = (uint32_t)lane_id() | first << 6;  // (r < 64; read after fill's barriers)
    }
    __device__ __forceinline__ void fill(uint32_t from) {  // from: a multiple of 64
        b0 = from;
        __syncthreads();  // the previous rounds' words are read
        if (lane_id() < OWNER_WORDS) hw[lane_id()] = 0;
        __syncthreads();
        const uint32_t r = (first - from) >> 6;
        if (has && first >= from && r < (uint32_t)OWNER_WORDS)
            atomicOr(reinterpret_cast<unsigned long long*>(hw + r), 1ull << (first & 63u));
        __syncthreads();
    }
    // fill before the rounds [g0, g0 + 64 OWNER_WORDS) of a pass that starts at item 0
    __device__ __forceinline__ void fill_at(uint32_t g0) {
        if ((g0 >> 6) % (uint32_t)OWNER_WORDS == 0) fill(g0);
    }
    // The owner lane of item g0 + lane (g0 a filled round's first item,
    // wave-uniform, below the pass's total: the rank is then at least 1) and
    // that lane's first item.
    __device__ __forceinline__ int owner(uint32_t g0, uint32_t& ofirst) const {
        const uint32_t K = (uint32_t)__popcll(__ballot(has && first < g0));
        const uint32_t e = tab[owner_rank(K, hw[(g0 - b0) >> 6], lane_id()) - 1u];
        ofirst = e >> 6;
        return (int)(e & 63u);
    }
};

// Per lane: the line's URI sources.  sp[u] = a | b << 16 (line-relative, 0 =
// none), cs[u] = the compact buffer offset of line byte a.  NU: the URI
// stages this kernel instance handles (>= P.n_uri; most programs have at
// most two, whose per-lane arrays then take two registers each)
template <int NU>
struct UriLane {
    bool ok;
    int fmt;
    uint64_t ls;  // line start in the input
    RegArr<NU> sp, cs, usep;
};

template <int NU>
__device__ __forceinline__ UriLane<NU> uri_lane(const Program& P, const Columns& C, int64_t li, bool active) {
    UriLane<NU> U;
    U.sp.fill(0);
    U.cs.fill(0);
    U.usep.fill(0);
    U.ok = false;
    U.fmt = 0;
    U.ls = 0;
    if (!active) return U;
    // every column read issued before the status is known (one round trip;
    // the values of a line that is not OK are not used)
    const uint8_t st = C.status[li];
    const int fmt = P.n_fmt > 1 ? (int)C.fmt_id[li] : 0;
    U.ls = C.line_off[li];
    const uint32_t tf = C.tok_flags[li];
    uint32_t raw[NU], kind[NU];
    for (int u = 0; u < NU; ++u) {
        raw[u] = 0;
        kind[u] = FL_FULL;
        if (u >= P.n_uri || P.uri[u].src_q >= 0) continue;
        if (P.uri[u].src_tok >= 0) {
            raw[u] = C.tok_span[P.uri[u].src_tok][li];
            kind[u] = (tf >> P.uri[u].src_tok) & 1u ? FL_NONE : FL_FULL;  // "-" -> null
        } else {
            raw[u] = C.fl_uri[P.uri[u].src_fl][li];
            kind[u] = C.fl_kind[P.uri[u].src_fl][li];
        }
    }
    U.ok = st == ST_OK;
    U.fmt = U.ok ? fmt : 0;
    if (U.ok)
        for (int u = 0; u < P.n_uri && u < NU; ++u) {
            // uri_source_cols (lp_device.h) on the values read above
            const int a = (int)(raw[u] & 0xFFFF), b = (int)(raw[u] >> 16);
            if (P.uri[u].fmt == U.fmt && P.uri[u].src_q < 0 && kind[u] != FL_NONE && b > a) U.sp.set(u, mkspan(a, b));
        }
    return U;
}


// The fast walk of URI stage u (lp_device.h uri_walk_fast) for all lines of
// the wave at once.  A line's event bytes (its UEV bits in [a, b), usep of
// them) are numbered line after line; each round, every lane takes one event
// of the wave: its byte, its class, and from ballots over its line's earlier
// events in the round plus the line's carried state (the owner lane's
// registers) what the sequential walk would know there -- whether an
// earlier event stopped the walk, the first '&' / '?' (fa), the previous
// query-piece boundary, the last '%' / '+'.  A boundary event that ends a
// non-empty piece writes its table slot; at the end of each round every
// owner lane folds its events of the round into its state.  The result per
// lane (part: the lane's line takes part) is exactly the sequential walk's
// state: resume, fa, first_pct, rewr bit 1, the query table (slots, count,
// s, lp).  L: the lane's line view (compact buffer with its UEV plane);
// A.p / A.used: the line's region and where its table starts.
template <typename CL>
__device__ __forceinline__ void uri_walk_coop(const Program& P, int u, const CL& L, bool part, int a, int b,
                                              uint32_t usep, const Arena& A, uint64_t* heads, UriWalk& Wk) {
    const int lane = lane_id();
    const bool table = P.uri[u].want_query && P.uri[u].query_stage >= 0;  // (wave-uniform)
    const uint32_t cnt = part ? usep : 0u;
    const uint32_t x = wave_incl_scan_dpp(cnt);
    const uint32_t eb = x - cnt, E = lane_value(x, 63);
    OwnerRounds OW(heads, eb, cnt);
    const uint32_t tab = (A.used + 15) & ~15u;
    const unsigned long long reg = (unsigned long long)(uintptr_t)A.p;
    // the owner's state (this lane's line)
    int resume = -1, fa = -1, fpct = -1, lastB = -1, lastPP = -1;
    uint32_t count = 0;
    bool rw = false;
    for (uint32_t g0 = 0; g0 < E; g0 += PW) {
        const uint32_t g = g0 + (uint32_t)lane;
        const bool valid = g < E;
        OW.fill_at(g0);
        uint32_t ebo;  // the owner's first event
        const int ow = OW.owner(g0, ebo);  // last lane whose first event is <= g
        const uint32_t oo = (uint32_t)__shfl((int)L.o, ow);
        const int oa = __shfl(a, ow), ob = __shfl(b, ow);
        // the event: the (g - ebo)-th UEV bit of the owner's [oa, ob)
        uint32_t Aq = 0;
        if (valid) {
            const uint32_t A0 = oo + (uint32_t)oa, A1 = oo + (uint32_t)ob, WL = (A1 - 1) >> 6;
            uint32_t W = A0 >> 6, k = g - ebo;
            uint64_t m = L.mask(MC_UEV, W) & (~0ull << (A0 & 63));
            for (;;) {
                if (W == WL) m &= ~0ull >> (63 - ((A1 - 1) & 63));
                const uint32_t c = (uint32_t)__popcll(m);
                if (k < c || W >= WL) break;  // (the count came from the same plane: k < c by WL)
                k -= c;
                ++W;
                m = L.mask(MC_UEV, W);
            }
            Aq = (W << 6) + select64(m, k);
        }
        const int q = (int)(Aq - oo);
        CL Lo = L;
        Lo.o = oo;
        Lo.n = ob;
        const uint32_t w = valid ? load_u32_at(Lo, q) : 0u;
        const uint32_t c = w & 0xFFu;
        const bool pct = c == '%';
        const bool bad_pct = pct && (q + 2 >= ob || !is_hex((w >> 8) & 0xFFu) || !is_hex((w >> 16) & 0xFFu));
        const bool stop = valid && (c == '#' || c == ';' || c >= 0x80 || bad_pct);
        const bool aq = c == '&' || c == '?';
        // the owner's state before this round
        const int cres = __shfl(resume, ow), cfa = __shfl(fa, ow), clB = __shfl(lastB, ow), clPP = __shfl(lastPP, ow);
        const uint32_t ccount = (uint32_t)__shfl((int)count, ow);
        // my line's earlier events in this round: lanes [seg0, lane)
        const int s0 = (int)ebo - (int)g0;
        const uint64_t below = (1ull << lane) - 1ull;
        const uint64_t seg_lt = valid ? below & (~0ull << (s0 > 0 ? s0 : 0)) : 0ull;
        const uint64_t Bstop = __ballot(stop);
        const bool live = valid && !stop && cres < 0 && !(Bstop & seg_lt);  // the fast walk takes this event
        const uint64_t Baq = __ballot(live && aq);
        const uint64_t mfa = Baq & seg_lt;
        const int qfa = __shfl(q, mfa ? lsb64(mfa) : lane);
        const int fa_j = cfa >= 0 ? cfa : (mfa ? qfa : -1);  // the first '&' / '?' before me
        const bool pp = live && ((pct && !bad_pct) || c == '+');
        const bool isB = table && live && aq && fa_j >= 0;  // a piece boundary after fa
        const uint64_t BB = __ballot(isB), BPP = __ballot(pp);
        const uint64_t mB = BB & seg_lt, mP = BPP & seg_lt;
        const int qpb = __shfl(q, mB ? msb64(mB) : lane), qpp = __shfl(q, mP ? msb64(mP) : lane);
        const bool first_piece = !mB && clB < 0;  // the previous boundary is fa
        const int pb = mB ? qpb : (clB >= 0 ? clB : fa_j);
        const int lpp = mP ? qpp : clPP;  // the last '%' / '+' before me
        const int lp = first_piece ? lpp : (lpp > pb ? lpp : -1);
        const bool emit = isB && q > pb + 1;
        const uint64_t BE = __ballot(emit);
        const bool rwj = live && fa_j >= 0 && ((aq && c == '?') || (!aq && !pct && uri_needs_encode(c)));
        const uint64_t BR = __ballot(rwj);
        const unsigned long long oreg = __shfl(reg, ow);
        const uint32_t otab = (uint32_t)__shfl((int)tab, ow);
        if (emit) {
            const uint32_t idx = ccount + (uint32_t)__popcll(BE & seg_lt);
            const uint64_t t0 = (uint64_t)(uint32_t)(pb + 1) | ((uint64_t)(uint32_t)q << 16) | ((uint64_t)(uint32_t)(lp + 1) << 48);
            *reinterpret_cast<LP_G u32x4*>(reinterpret_cast<LP_G uint8_t*>(oreg) + otab + 16 * idx) =
                u32x4{(uint32_t)t0, (uint32_t)(t0 >> 32), 0u, 0u};
        }
        // owners fold their events of this round into their state
        const int so = (int)eb - (int)g0, eo = (int)(eb + cnt) - (int)g0;
        const int so_c = so < 0 ? 0 : so > PW ? PW : so, eo_c = eo < 0 ? 0 : eo > PW ? PW : eo;
        const uint64_t segm = so_c < eo_c ? ((eo_c == PW ? ~0ull : (1ull << eo_c) - 1ull) & (~0ull << so_c)) : 0ull;
        const uint64_t ms = Bstop & segm, mf = Baq & segm, mpct = __ballot(live && pct) & segm, mb = BB & segm,
                       mpp = BPP & segm;
        const int q_s = __shfl(q, ms ? lsb64(ms) : lane), q_f = __shfl(q, mf ? lsb64(mf) : lane);
        const int q_p = __shfl(q, mpct ? lsb64(mpct) : lane), q_b = __shfl(q, mb ? msb64(mb) : lane);
        const int q_pp = __shfl(q, mpp ? msb64(mpp) : lane);
        if (resume < 0 && ms) resume = q_s;
        if (fa < 0 && mf) fa = q_f;
        if (fpct < 0 && mpct) fpct = q_p;
        if (mb) lastB = q_b;
        if (mpp) lastPP = q_pp;
        count += (uint32_t)__popcll(BE & segm);
        rw = rw || (BR & segm) != 0;
    }
    if (!part) return;
    Wk.resume = resume;
    Wk.fa = fa;
    Wk.first_pct = fpct;
    Wk.rewr = rw ? 2u : 0u;
    QueryTable& T = Wk.T;
    if (table && fa >= 0) {
        T.on = T.set = true;
        T.maxp = usep + 1;
        T.tab = tab;
        T.reg = tab + 16 * T.maxp;
        T.s = (lastB >= 0 ? lastB : fa) + 1;
        T.count = count;
        T.lp = lastB >= 0 ? (lastPP > lastB ? lastPP : -1) : lastPP;
    } else {
        T.lp = lastPP;
    }
}

// Query values waiting for the piece pass's dense decode (uri_wave): a piece
// whose value holds a '%' / '+' is decoded by a lane of its own, not by the
// lane that holds the piece.  That lane posts a descriptor -- the value's
// source bytes [S, E) as offsets from its view's base, where the output
// starts in the owning line's region (used), that region (reg: its offset
// from the wave's first region) and the piece's table slot in it (soff) --
// and lane d of a decode pass takes descriptor d.  A piece whose value holds
// a '%' / '+' but is not decoded (its name is not requested, or its spill did
// not fit) posts an empty descriptor: a block's descriptors are numbered
// before its names are looked at.  URI_CAPD descriptors fit the buffer: one
// pass' worth, and any one block's.  A view in LDS (the compact buffer, one
// base for the wave) takes 16 bytes, a view in HBM carries its line's base
// pointer and takes 32.
constexpr int URI_CAPD = PW;
constexpr uint32_t QDESC_NONE = ~0u;  // soff of an empty descriptor
template <typename LN>
struct QDescs {
    static constexpr int WORDS = LN::has_masks ? 2 : 4;  // uint64_t per descriptor
    uint64_t* buf;  // 16-byte aligned, URI_CAPD * WORDS words
    __device__ __forceinline__ void post(uint32_t d, const LN& OL, int vs, int e, uint32_t used, uint32_t reg,
                                         uint32_t soff) const {
        const uint32_t S = OL.o + (uint32_t)vs, E = OL.o + (uint32_t)e;
        u32x4* q = reinterpret_cast<u32x4*>(buf + WORDS * d);
        if constexpr (LN::has_masks) {
            q[0] = u32x4{S | E << 16, used, reg, soff};  // (S <= E <= 0xFFFF: the compact buffers are smaller)
        } else {
            const unsigned long long b = (unsigned long long)(uintptr_t)OL.b;
            q[0] = u32x4{S, E, reg, soff};
            q[1] = u32x4{(uint32_t)b, (uint32_t)(b >> 32), used, 0u};
        }
    }
    __device__ __forceinline__ void post_none(uint32_t d) const {
        *reinterpret_cast<u32x4*>(buf + WORDS * d) = u32x4{0u, 0u, 0u, QDESC_NONE};
    }
    // Descriptor d: V views the value's bytes [S, E) (V.o = 0; the view ends
    // with the value, whose decoder reads no word that starts at or after E:
    // every escape of a piece lies inside it).  L0: any view of the wave's
    // (the LDS base).  false: an empty descriptor.
    __device__ __forceinline__ bool take(uint32_t d, const LN& L0, LN& V, int& S, int& E, uint32_t& used, uint32_t& reg,
                                         uint32_t& soff) const {
        const u32x4* q = reinterpret_cast<const u32x4*>(buf + WORDS * d);
        const u32x4 a = q[0];
        V = L0;
        V.o = 0;
        reg = a[2];
        soff = a[3];
        if constexpr (LN::has_masks) {
            S = (int)(a[0] & 0xFFFFu);
            E = (int)(a[0] >> 16);
            used = a[1];
        } else {
            const u32x4 c = q[1];
            V.b = reinterpret_cast<decltype(V.b)>((uintptr_t)((unsigned long long)c[0] | (unsigned long long)c[1] << 32));
            S = (int)a[0];
            E = (int)a[1];
            used = c[2];
        }
        V.n = E;
        return soff != QDESC_NONE;
    }
};

// Phase 2, the arena allocation and the query pieces of one wave; lu(u) is
// the lane's line view of URI stage u (valid for every lane, empty stages
// included: the query pass reads other lanes' views).
// A line whose URI the reference repairs (ST_REPAIR) is stored as FALLBACK;
// QUEUE: it is appended to uri_fix_list (k_uri_lines), else `redo` tells the
// caller to redo it (k_uri_overflow, which also works the list off).
// scratch: LDS for the piece pass's descriptors (QDescs), the kernels' UEV
// plane: the walks and uri_stage_rest are its last readers (nothing after
// LP_PROF(21) calls a view's mask(): query_prep, query_name and
// url_decode_value read bytes and words only), and the direct path never
// reads it.
template <int NU, int NQ, bool COOP, bool QUEUE, typename LU, typename LL>
__device__ __forceinline__ void uri_wave(const Program& P, const Columns& C, UriLane<NU>& U, LU&& lu, LL&& ll,
                                         bool active, int64_t li, int64_t wave, uint64_t* heads, uint64_t* scratch,
                                         WaveCounts& WC, bool& redo) {
    const int lane = lane_id();
    const int nq = P.n_query < NQ ? P.n_query : NQ;
    uint32_t need = 0;
    if (U.ok)
        for (int u = 0; u < P.n_uri && u < NU; ++u) {
            const uint32_t s = U.sp.get(u);
            if (!s) continue;
            uint32_t ev;
            need += uri_need(P, u, lu(u), (int)(s & 0xFFFF), (int)(s >> 16), ev);
            U.usep.set(u, ev);
        }
    // upstream list stages (UpstreamListDissector): their item tables follow
    // the URI stages' in the line's region (and the name / value pieces of
    // cookie headers and raw query strings); ll(lend) views the list / pair
    // token bytes (gathered into LDS beside the URI bytes, or in HBM)
    int lend = 0;
    if (U.ok) {
        for (int j = 0; j < P.n_list; ++j)
            if (P.list[j].fmt == U.fmt) lend = max(lend, (int)(C.tok_span[P.list[j].tok][li] >> 16));
        for (int j = 0; j < P.n_pair; ++j)
            if (P.pair[j].fmt == U.fmt) lend = max(lend, (int)(C.tok_span[P.pair[j].tok][li] >> 16));
    }
    if (lend) ll(lend, [&](const auto& LH) { need += list_need(P, U.fmt, LH, C, li) + pair_need(P, U.fmt, LH, C, li); });
    need = (need + 15) & ~15u;
    // wave-aggregated arena allocation from the wave's shard
    LP_PROF(29);
    const uint32_t x = wave_incl_scan_dpp(need);
    const uint32_t total = lane_value(x, 63);
    LP_PROF(20);
    const int shard = (int)(wave % ARENA_SHARDS);
    unsigned long long wbase = 0;
    // regions start 16-byte aligned (their query tables take 16-byte slot
    // stores; spills keep the bump pointer only 4-byte aligned)
    if (lane == 63 && total) wbase = atomicAdd(&C.meta->shard_top[16 * shard], (unsigned long long)total + 12ull);
    // (read as scalars: the wave's base is kept for the piece pass's descriptors)
    wbase = (((unsigned long long)lane_value((uint32_t)wbase, 63) | (unsigned long long)lane_value((uint32_t)(wbase >> 32), 63) << 32) + 15) & ~15ull;
    const bool fits = wbase + total <= C.shard_cap;
    LP_PROF(26);
    uint32_t written = 0;
    unsigned long long my_region = 0;
    UriOutT<NQ> o;
    o.qlist.fill(0);
    o.qpend.fill(0);
    o.status = U.ok ? ST_OK : ST_BAD;
    Arena A{C.arena, 0, 0};
    bool live = false;  // the line's region is allocated: phase 2 runs
    if (U.ok) {
        if (!fits && need) {
            // the shard is full: the batch is re-run with a larger arena
            o.status = ST_FALLBACK;
            atomicAdd(&C.meta->arena_ovf, 1ull);
        } else {
            const unsigned long long mine = (unsigned long long)shard * C.shard_cap + wbase + x - need;
            my_region = mine;
            C.arena_base[li] = mine;  // also for an empty region: spills are region-relative
            A = Arena{C.arena + mine, 0, need};
            A.top = &C.meta->shard_top[16 * shard];  // spills come from the same shard
            A.base = wbase + x - need;
            A.limit = C.shard_cap;
            live = true;
        }
    }
    // phase 2 (lp_device.h phase2), stage by stage for the whole wave: the
    // compact path walks the stages' event bytes cooperatively
    const int nu = P.n_uri < NU ? P.n_uri : NU;
    for (int u = 0; u < nu; ++u) {
        const bool fmt_ok = live && o.status == ST_OK && P.uri[u].fmt == U.fmt;
        const uint32_t sp = U.sp.get(u);
        const int a = (int)(sp & 0xFFFF), b = (int)(sp >> 16);
        const bool part = fmt_ok && b > a;
        if (fmt_ok && !part) {
            C.u_flags[u][li] = 0;
            if (P.uri[u].query_stage >= 0) { C.q_count[P.uri[u].query_stage][li] = 0; C.q_params[P.uri[u].query_stage][li] = 0; }
        }
        LP_PROF(10 + 2 * u);
        UriWalk Wk;
        if constexpr (COOP) {
            LP_PROF(50 + 4 * u);
            uri_walk_coop(P, u, lu(u), part, a, b, U.usep.get(u), A, heads, Wk);
            LP_PROF(51 + 4 * u);
        } else if (part) {
            uri_walk_fast(P, u, lu(u), a, b, U.usep.get(u), A, Wk);
        }
        if (part) {
            const int st = uri_stage_rest<UR_OFF>(P, u, lu(u), a, b, U.usep.get(u), A, C, li, o, Wk);
            if (st != ST_OK) o.status = st;  // (ST_REPAIR too: settled where the status is stored)
        }
        LP_PROF(11 + 2 * u);
    }
    if (live && lend && o.status == ST_OK) {
        bool filled = true;
        ll(lend, [&](const auto& LH) { filled = list_fill(P, U.fmt, LH, A, C, li) && pair_fill(P, U.fmt, LH, A, C, li); });
        if (!filled) o.status = ST_FALLBACK;
    }
    if (live) {
        if (A.ovf) {
            o.status = ST_FALLBACK;
            atomicAdd(&C.meta->arena_ovf, 1ull);
        }
        written = A.used - A.slack + A.extra;
    }
    LP_PROF(21);
    // QueryStringFieldDissector pieces of all lines of the wave, spread evenly
    // over the lanes (a line's pieces vary from 0 to dozens; one lane per line
    // would leave most lanes idle while the longest query finishes): the
    // pieces of every query stage in one numbering (a lane's stage-0 pieces,
    // then its stage-1 pieces, ...), QR blocks of 64 pieces per round: their
    // table slots loaded together, then query_prep, ONE spill allocation for
    // the round, query_finish's name part where the piece is and its decode
    // on dense lanes.  Most waves need one round for all stages.
    if (nq > 0) {
        constexpr int QR = LP_URI_QR;
        __syncthreads();  // the table slots written in phase 2 are visible to every lane
        const bool has = U.ok && o.status == ST_OK && need != 0;
        const unsigned long long my_ab = has ? my_region : 0ull;
        uint64_t piece_ovf = 0;  // lanes whose line lost a piece for want of arena
        uint32_t np = 0;
        for (int qs = 0; qs < nq; ++qs) np += has ? o.qpend.get(qs) : 0u;
        const uint32_t incl = wave_incl_scan_dpp(np);
        const uint32_t base = incl - np, tot = lane_value(incl, 63);
        OwnerRounds OW(heads, base, np);
        // piece j of lane ow: its query stage and its slot in ow's region;
        // OL = ow's line view of that stage (every lane takes part in the shuffles)
        auto piece = [&](int ow, uint32_t j, int& pq, uint32_t& soff) {
            uint32_t cum = 0;
            pq = 0;
            soff = 0;
            for (int qs = 0; qs < nq; ++qs) {
                const uint32_t c = (uint32_t)__shfl((int)(has ? o.qpend.get(qs) : 0u), ow);
                const uint32_t l = (uint32_t)__shfl((int)o.qlist.get(qs), ow);
                if (j >= cum && j < cum + c) {
                    pq = qs;
                    soff = l + 16 * (j - cum);
                }
                cum += c;
            }
        };
        auto owner_view = [&](int ow, int pq) {
            auto OL = owner_line(lu(P.query[0].uri), ow);
            for (int qs = 1; qs < nq; ++qs) {
                const auto V = owner_line(lu(P.query[qs].uri), ow);
                if (pq == qs) OL = V;
            }
            return OL;
        };
        // The dense decode pass: lane d decodes the d-th waiting value
        // (url_decode_value, as query_finish runs it: the same bytes, the
        // last word's padding included) and stores its ref in the piece's
        // slot.  Every owner is a line of this wave: its region lies at reg
        // after the wave's first.  Wave-uniform control flow; workgroups are
        // one wave, the barriers only order the LDS accesses.
        typedef decltype(lu(0)) QL;
        const QDescs<QL> QD{scratch};
        const unsigned long long w0 = (unsigned long long)shard * C.shard_cap + wbase;  // the wave's first region
        LP_G uint8_t* const wreg = C.arena + w0;
        auto decode_waiting = [&](uint32_t n) {
            LP_PT_DECL
            __syncthreads();  // the descriptors posted are visible
            if ((uint32_t)lane < n) {
                QL V;
                int S, E;
                uint32_t used, reg, soff;
                if (QD.take((uint32_t)lane, lu(P.query[0].uri), V, S, E, used, reg, soff)) {
                    Arena A{wreg + reg, used, used};
                    reinterpret_cast<LP_G uint64_t*>(wreg + reg + soff)[1] = url_decode_value(V, S, E, A);
                    written += A.used - used;
                }
            }
            __syncthreads();  // ... and read before the next are posted
            LP_PACC(57);
        };
        for (uint32_t g0 = 0; g0 < tot; g0 += QR * PW) {
            int own[QR], pqs[QR];
            uint32_t soffs[QR];
            uint64_t t0[QR];
#pragma unroll
            for (int k = 0; k < QR; ++k) {
                own[k] = 0;
                pqs[k] = 0;
                soffs[k] = 0;
                t0[k] = 0;
                if (g0 + (uint32_t)(k * PW) >= tot) continue;  // no piece in this block (uniform)
                const uint32_t g = g0 + (uint32_t)(k * PW + lane);
                OW.fill_at(g0 + (uint32_t)(k * PW));
                uint32_t ob;  // the owner's first pending piece index
                const int ow = OW.owner(g0 + (uint32_t)(k * PW), ob);  // last lane whose first piece index is <= g
                own[k] = ow;
                const unsigned long long oab = __shfl(my_ab, ow);
                piece(ow, g - ob, pqs[k], soffs[k]);
                if (g < tot) t0[k] = *reinterpret_cast<const LP_G uint64_t*>(C.arena + oab + soffs[k]);
            }
            LP_PROF(17);
            QPrep qp[QR];
            uint32_t mine = 0;
#pragma unroll
            for (int k = 0; k < QR; ++k) {
                if (g0 + (uint32_t)(k * PW) >= tot) continue;
                const uint32_t g = g0 + (uint32_t)(k * PW + lane);
                const auto OL = owner_view(own[k], pqs[k]);
                if (g < tot) qp[k] = query_prep(OL, t0[k]);
                mine += qp[k].need;
            }
            LP_PROF(18);
            // the round's spilled bytes in one allocation from the wave's
            // shard (every owner is a line of this wave)
            const uint32_t x = wave_incl_scan_dpp(mine);
            const uint32_t rtot = lane_value(x, 63);
            unsigned long long rbase = 0;
            if (lane == 63 && rtot) rbase = atomicAdd(&C.meta->shard_top[16 * shard], (unsigned long long)rtot);
            unsigned long long at = __shfl(rbase, 63) + x - mine;  // this lane's first piece in the shard
            LP_PROF(19);
            // query_finish, in two parts: the lane that holds a piece does the
            // name part (query_name) and the values that need no decoding; a
            // piece whose value does (qp.pv) it posts for the dense decode
            // pass, at its rank among the block's such pieces after those
            // already waiting.  Waiting values are decoded when a block's
            // would not fit with them, and after the round's last block.
            uint32_t nwait = 0;  // (wave-uniform)
#pragma unroll
            for (int k = 0; k < QR; ++k) {
                if (g0 + (uint32_t)(k * PW) >= tot) continue;
                const uint32_t g = g0 + (uint32_t)(k * PW + lane);
                const bool pv = g < tot && qp[k].pv;
                const uint64_t PB = __ballot(pv);
                const uint32_t nb = (uint32_t)__popcll(PB);
                if (nwait + nb > (uint32_t)URI_CAPD) {
                    decode_waiting(nwait);
                    nwait = 0;
                }
                const uint32_t d = nwait + __builtin_amdgcn_mbcnt_hi((uint32_t)(PB >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)PB, 0u));
                nwait += nb;
                const int ow = own[k];
                const unsigned long long oab = __shfl(my_ab, ow);
                const auto OL = owner_view(ow, pqs[k]);
                bool povf = false;
                if (g < tot) {
                    LP_G uint64_t* slot = reinterpret_cast<LP_G uint64_t*>(C.arena + oab + soffs[k]);
                    const unsigned long long rel = oab - (unsigned long long)shard * C.shard_cap;  // region in the shard
                    if (qp[k].need && (at + qp[k].need > C.shard_cap || at - rel + qp[k].need > 0x7FFFFFFFull)) {
                        slot[0] = REF_SKIP;
                        slot[1] = 0;
                        povf = true;
                        if (pv) QD.post_none(d);
                        atomicAdd(&C.meta->arena_ovf, 1ull);  // the batch is re-run with a larger arena
                    } else {
                        Arena A{C.arena + oab, (uint32_t)(at - rel), (uint32_t)(at - rel + qp[k].need)};
                        const uint32_t a1 = A.used;
                        uint64_t nref;
                        const bool want = query_name(P, P.query[pqs[k]], OL, A, C.arena + oab, qp[k], nref);
                        if (!want) {
                            slot[0] = REF_SKIP;
                            slot[1] = 0;
                        } else {
                            slot[0] = nref;
                            if (!pv) slot[1] = query_value_plain(OL, qp[k]);
                        }
                        // (A.used: after the aligned name part, where the value's output starts)
                        if (pv) QD.post(d, OL, qp[k].eq + 1, qp[k].e, A.used, (uint32_t)(oab - w0), want ? soffs[k] : QDESC_NONE);
                        written += A.used - a1;
                    }
                    at += qp[k].need;
                }
                // a piece that did not fit: its line goes to FALLBACK (the
                // batch is re-run with a larger arena, or, when the re-runs
                // are spent, delivered with those lines FALLBACK)
                for (uint64_t m = __ballot(povf); m; m &= m - 1) piece_ovf |= 1ull << __shfl(ow, (int)__builtin_ctzll(m));
            }
            if (nwait) decode_waiting(nwait);
        }
        if (((piece_ovf >> lane) & 1) && o.status == ST_OK) o.status = ST_FALLBACK;
    }
    LP_PROF(22);
    redo = false;
    if (U.ok && o.status == ST_REPAIR) {
        // a malformed URI the reference repairs: FALLBACK until the line is redone
        o.status = ST_FALLBACK;
        if constexpr (QUEUE) {
            const unsigned long long k = atomicAdd(&C.meta->uri_fix_lines, 1ull);
            if (k < (unsigned long long)C.cap_lines) C.uri_fix_list[k] = (uint32_t)li;
        } else {
            redo = true;
        }
    }
    if (U.ok && o.status != ST_OK) C.status[li] = (uint8_t)o.status;
    for (int d = 32; d > 0; d >>= 1) written += __shfl_xor(written, d);
    const int st = !active ? -1 : U.ok ? o.status : (int)C.status[li];
    WC.act += (uint32_t)__popcll(__ballot(active));
    WC.ok += (uint32_t)__popcll(__ballot(st == ST_OK));
    WC.bad += (uint32_t)__popcll(__ballot(st == ST_BAD));
    WC.written += written;
}


// The URI stages of one wave on the compact path: its lines' URI bytes
// gathered into cbuf (CAP bytes) with their UEV plane, then uri_wave.
// Returns false, having done nothing, when the wave's bytes exceed CAP.
template <int NU, int NQ, uint32_t CAP>
__device__ __forceinline__ bool uri_compact(const uint8_t* __restrict__ buf, uint64_t nbytes, const Program& P,
                                            const Columns& C, int64_t wave, int64_t n_lines, uint32_t* cbuf,
                                            uint64_t* plane, uint64_t* heads, WaveCounts& WC, bool& redo) {
    const int lane = lane_id();
    const int64_t li = wave * PW + lane;
    const bool active = li < n_lines;
    LP_PROF(23);
    UriLane<NU> U = uri_lane<NU>(P, C, li, active);
    LP_PROF(27);
    // one region per line: the 16-byte input blocks holding all its URI
    // sources (request URI, referer, ...: close together in a line), in
    // line order; a block keeps its alignment, so the wave gathers whole
    // aligned 16-byte blocks, consecutive lanes taking consecutive blocks
    uint64_t lo = ~0ull, hi = 0;
    for (int u = 0; u < P.n_uri && u < NU; ++u) {
        const uint32_t s = U.sp.get(u);
        if (!s) continue;
        lo = min(lo, U.ls + (s & 0xFFFF));
        hi = max(hi, U.ls + (s >> 16));
    }
    const uint64_t r0 = hi ? lo & ~15ull : 0;
    const uint32_t nb1 = hi ? (uint32_t)((((hi + 15) & ~15ull) - r0) >> 4) : 0u;
    // the line's list / pair tokens (upstream lists, cookie headers, raw
    // query strings): a second region of blocks after the URI ones
    const bool lists = P.n_list > 0 || P.n_pair > 0;  // wave-uniform
    uint64_t l0 = ~0ull, l1 = 0;
    if (lists && U.ok) {
        auto add = [&](int tok) {
            const uint32_t s = C.tok_span[tok][li];
            if ((s >> 16) > (s & 0xFFFFu)) {
                l0 = min(l0, U.ls + (s & 0xFFFFu));
                l1 = max(l1, U.ls + (s >> 16));
            }
        };
        for (int j = 0; j < P.n_list; ++j)
            if (P.list[j].fmt == U.fmt) add(P.list[j].tok);
        for (int j = 0; j < P.n_pair; ++j)
            if (P.pair[j].fmt == U.fmt) add(P.pair[j].tok);
    }
    const uint64_t q0 = l1 ? l0 & ~15ull : 0;
    const uint32_t nb2 = l1 ? (uint32_t)((((l1 + 15) & ~15ull) - q0) >> 4) : 0u;
    auto blocks = [&](uint32_t n, uint32_t& first) {  // the wave's block count, this line's first block
        const uint32_t x = wave_incl_scan_dpp(n);
        first = x - n;
        return lane_value(x, 63);
    };
    uint32_t cb, nb = nb1 + nb2;  // this line's blocks
    uint32_t tot = blocks(nb, cb);
    // the list / pair tokens in LDS when the wave's bytes fit with them, else
    // read from HBM (only the URI bytes decide whether the wave fits)
    bool lin = lists;
    if (lists && 16 * tot + 16 > CAP) {
        lin = false;
        nb = nb1;
        tot = blocks(nb, cb);
    }
    if (16 * tot + 16 > CAP) return false;
    WC.gathered = 16 * tot;
    for (int u = 0; u < P.n_uri && u < NU; ++u) {
        const uint32_t s = U.sp.get(u);
        if (s) U.cs.set(u, 16 * cb + (uint32_t)(U.ls + (s & 0xFFFF) - r0));
    }
    // gather: block g of the wave is block g - cb[own] of line own's region,
    // own = the last lane whose first block is <= g (OwnerRounds: a batch's
    // head masks filled at once); every round's load in flight before the
    // first store
    constexpr int GR = LP_URI_GR;  // rounds per batch (the main kernel's CAP / 1024, rounded up)
    uint16_t* pl16 = reinterpret_cast<uint16_t*>(plane);
    OwnerRounds OW(heads, cb, nb);
    for (uint32_t g0 = 0; g0 < tot; g0 += GR * PW) {
        u32x4 v[GR];
        OW.fill(g0);
#pragma unroll
        for (int k = 0; k < GR; ++k) {
            v[k] = u32x4{0, 0, 0, 0};
            if (g0 + (uint32_t)(k * PW) >= tot) continue;  // no block in this round (uniform)
            const uint32_t g = g0 + (uint32_t)(k * PW + lane);
            uint32_t ocb;  // the owner's first block
            const int own = OW.owner(g0 + (uint32_t)(k * PW), ocb);
            const uint32_t j = g - ocb;  // block j of line own's regions
            uint64_t src = (uint64_t)__shfl((unsigned long long)r0, own) + 16ull * j;
            if (lin) {  // (every lane in the shuffles: a permute reads no value from an inactive lane)
                const uint32_t n1 = (uint32_t)__shfl(nb1, own);
                const uint64_t s1 = (uint64_t)__shfl((unsigned long long)q0, own);
                if (j >= n1) src = s1 + 16ull * (j - n1);
            }
            if (g < tot) v[k] = load16(buf, nbytes, src);
        }
        LP_PROF(28);
#pragma unroll
        for (int k = 0; k < GR; ++k) {
            const uint32_t g = g0 + (uint32_t)(k * PW + lane);
            if (g >= tot) continue;
            *reinterpret_cast<u32x4*>(cbuf + 4 * g) = v[k];
            pl16[g] = (uint16_t)bcls::classify16u(v[k][0], v[k][1], v[k][2], v[k][3]);
        }
    }
    LP_PROF(24);
    // one zero block after the last (the scanners' look-ahead word) and the
    // rest of the last 64-byte mask block
    for (uint32_t g = tot + lane; g < ((tot + 1 + 3) & ~3u); g += PW) {
        *reinterpret_cast<u32x4*>(cbuf + 4 * g) = u32x4{0, 0, 0, 0};
        pl16[g] = 0;
    }
    __syncthreads();
    LP_PROF(25);
    typedef LineT<lds_bytes, lds_u64, 1> CL;
    auto lu = [&](int u) {
        const uint32_t s = U.sp.get(u);
        // line byte q lives at cbuf + cs + (q - a): origin cs - a (mod 2^32)
        return CL{(lds_bytes)cbuf, U.cs.get(u) - (s & 0xFFFFu), (int)(s >> 16), (lds_u64)plane};
    };
    // line byte q of a list / pair token at cbuf + 16 (cb + nb1) + (q - (q0 - ls)),
    // or in place in the input; ll(lend, f) runs f on the view (lin is
    // wave-uniform: LDS or global loads, never flat ones)
    const LP_G uint8_t* lsp = (const LP_G uint8_t*)buf + U.ls;
    const uint32_t lmis = (uint32_t)((uintptr_t)lsp & 3);
    const uint32_t lorig = 16 * (cb + nb1) + (uint32_t)(U.ls - q0);
    auto ll = [&](int lend, auto&& f) {
        if (lin) f(LineT<lds_bytes>{(lds_bytes)cbuf, lorig, lend});
        else f(LineT<const LP_G uint8_t*>{lsp - lmis, lmis, lend});
    };
    uri_wave<NU, NQ, true, CAP == URI_CAP>(P, C, U, lu, ll, active, li, wave, heads, plane, WC, redo);
    return true;
}

// 16 waves per CU: the LDS share allows them, and __launch_bounds__(64, 4)
// (4 waves per SIMD) keeps the registers within 128
template <int NU, int NQ>
__global__ __launch_bounds__(PW, 4) void k_uri_lines(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                     const DeviceArgs* __restrict__ args) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const int64_t wave = blockIdx.x;
    if (wave * PW >= n_lines || C.meta->cap_ovf) return;
    __shared__ __attribute__((aligned(16))) uint32_t cbuf[URI_CAP / 4 + 16];
    // (the UEV plane, then the piece pass's descriptors: 16-byte stores)
    __shared__ __attribute__((aligned(16))) uint64_t plane[URI_CAP / 64 + 1];
    static_assert(sizeof(plane) >= URI_CAPD * 16, "the plane holds URI_CAPD descriptors of the compact view");
    __shared__ uint64_t heads[OWNER_LDS_WORDS];  // (with cbuf and plane within 10,240 B: 16 workgroups per CU)
    WaveCounts WC;
    bool redo;  // (unused: this kernel queues such lines)
    if (uri_compact<NU, NQ, URI_CAP>(buf, nbytes, P, C, wave, n_lines, cbuf, plane, heads, WC, redo)) WC.store(C, wave);
    else if (lane_id() == 0) C.uri_ovf_list[atomicAdd(&C.meta->uri_ovf_waves, 1ull)] = (uint32_t)wave;
}

// Redoes line li, for which a URI kernel stored FALLBACK because a URI stage
// met a malformed URI that the reference repairs (lp_device.h uri_repair):
// the line read from HBM, its whole phase 2 serially (phase2 with the repair
// on, the query pieces, the list and pair stages) in a fresh region of the
// line's shard.  Stores the final status and corrects the owning wave's
// counts, which that wave has stored (atomics: the lanes here hold lines of
// different waves).  One line per lane, no wave-level operation inside.
__device__ __forceinline__ void uri_redo_line(const uint8_t* __restrict__ buf, uint64_t nbytes, const Program& P,
                                              const Columns& C, int64_t n_lines, int64_t li) {
    if ((uint64_t)li >= (uint64_t)n_lines) return;  // (never: the URI kernels name their own lines)
    const uint64_t s = C.line_off[li], e = C.line_off[li + 1] - 1;
    if (e < s || e - s > 0xFFFFull || e > nbytes) return;  // (never: the line passed phase 1)
    const int n = crlf_len((int)(e - s), e > s ? buf[e - 1] : 0u);
    const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + s;
    const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
    const LineT<const LP_G uint8_t*> L{ls - mis, mis, n};
    const int fmt = P.n_fmt > 1 ? (int)C.fmt_id[li] : 0;
    RegArr<MAX_URI> sp, usep;
    sp.fill(0);
    usep.fill(0);
    uint32_t need = 0;
    for (int u = 0; u < P.n_uri; ++u) {
        int a, b;
        if (P.uri[u].fmt != fmt || !uri_source_cols(P, C, li, u, a, b) || b > n) continue;
        uint32_t ev;
        need += uri_need(P, u, L, a, b, ev);
        sp.set(u, mkspan((uint32_t)a, (uint32_t)b));
        usep.set(u, ev);
    }
    need += list_need(P, fmt, L, C, li) + pair_need(P, fmt, L, C, li);
    need = (need + 15) & ~15u;
    // the fresh region: from the shard the line's wave allocates in
    // (regions start 16-byte aligned, the bump pointer is 4-byte aligned)
    const int shard = (int)((li / PW) % ARENA_SHARDS);
    LP_G unsigned long long* top = &C.meta->shard_top[16 * shard];
    const unsigned long long x = (atomicAdd(top, (unsigned long long)need + 12ull) + 15) & ~15ull;
    int st = ST_FALLBACK;
    uint32_t written = 0;
    if (x + need > C.shard_cap) {
        atomicAdd(&C.meta->arena_ovf, 1ull);  // the batch is re-run with a larger arena
    } else {
        const unsigned long long mine = (unsigned long long)shard * C.shard_cap + x;
        C.arena_base[li] = mine;
        Arena A{C.arena + mine, 0, need};
        A.top = top;
        A.base = x;
        A.limit = C.shard_cap;
        UriOut o;
        o.qlist.fill(0);
        o.qpend.fill(0);
        auto lu = [&](int) { return L; };
        phase2<UR_ON>(P, fmt, lu, sp, usep, o, A, C, li);
        if (o.status == ST_OK) query_pieces_serial(P, lu, o, A);
        if (o.status == ST_OK && (!list_fill(P, fmt, L, A, C, li) || !pair_fill(P, fmt, L, A, C, li))) o.status = ST_FALLBACK;
        if (A.ovf) {
            o.status = ST_FALLBACK;
            atomicAdd(&C.meta->arena_ovf, 1ull);
        }
        st = o.status;
        written = A.used - A.slack + A.extra;
    }
    // the URI kernel stored FALLBACK and counted the line so
    LP_G uint32_t* wc = C.wave_counts + WC_WORDS * (size_t)(li / PW);
    if (st != ST_FALLBACK) {
        C.status[li] = (uint8_t)st;
        atomicAdd(&wc[st == ST_OK ? 1 : 2], 1u);
        atomicSub(&wc[3], 1u);
    }
    if (written) atomicAdd(&wc[4], written);
}

// The waves k_uri_lines queued (their URI bytes exceed its compact buffer),
// on a persistent grid: the same path with a buffer four times as large (few
// waves: their occupancy does not matter), and for a wave exceeding even
// that, the lines' bytes read from HBM directly.  Then the lines k_uri_lines
// queued for uri_redo_line (its list is complete when this kernel starts),
// one per lane over the same grid: with an empty list, the usual case, that
// is one load.  A line of this kernel's own waves that needs the redo is
// redone by its lane at once, and counted in the upper half of
// Meta::uri_fix_lines (the lower half is the list's length, read by every
// block here).
constexpr uint32_t URI_CAP_OVF = 4 * URI_CAP;
template <int NU, int NQ>
__global__ __launch_bounds__(PW) void k_uri_overflow(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                     const DeviceArgs* __restrict__ args) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const uint64_t nq = C.meta->uri_ovf_waves;
    const uint64_t nfix = min((uint64_t)(uint32_t)C.meta->uri_fix_lines, (uint64_t)C.cap_lines);
    __shared__ __attribute__((aligned(16))) uint32_t cbuf[URI_CAP_OVF / 4 + 16];
    __shared__ __attribute__((aligned(16))) uint64_t plane[URI_CAP_OVF / 64 + 1];
    static_assert(sizeof(plane) >= URI_CAPD * 32 && URI_CAP_OVF + 64 <= 0xFFFF, "URI_CAPD descriptors of either view; 16-bit offsets");
    __shared__ uint64_t heads[OWNER_LDS_WORDS];
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t wave = C.uri_ovf_list[q];
        WaveCounts WC;
        bool redo = false;
        if (!uri_compact<NU, NQ, URI_CAP_OVF>(buf, nbytes, P, C, wave, n_lines, cbuf, plane, heads, WC, redo)) {
            const WaveLines W = wave_lines(C, wave, n_lines, nbytes);
            UriLane<NU> U = uri_lane<NU>(P, C, W.li, W.active);
            const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + W.s;
            const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
            const LineT<const LP_G uint8_t*> L{ls - mis, mis, crlf_len_hbm(buf, W)};
            auto lu = [&](int) { return L; };
            auto ll = [&](int lend, auto&& f) { f(LineT<const LP_G uint8_t*>{ls - mis, mis, lend}); };
            uri_wave<NU, NQ, false, false>(P, C, U, lu, ll, W.active, W.li, wave, heads, plane, WC, redo);
        }
        __syncthreads();
        WC.store(C, wave);
        if (__any(redo)) {
            __threadfence();  // the wave's counts are stored before a lane corrects them
            if (redo) {
                atomicAdd(&C.meta->uri_fix_lines, 1ull << 32);
                uri_redo_line(buf, nbytes, P, C, n_lines, wave * PW + lane_id());
            }
        }
    }
    for (uint64_t q = (uint64_t)blockIdx.x * PW + (uint64_t)lane_id(); q < nfix; q += (uint64_t)gridDim.x * PW)
        uri_redo_line(buf, nbytes, P, C, n_lines, (int64_t)C.uri_fix_list[q]);
}

// Derived URI stages (type-remapped query parameters, lp_device.h
// derived_line), after both URI kernels: one line per lane, the sources read
// in place (the input, or the decoded value in the line's region), every
// table and rewritten part spilled from the region's shard.  Only launched
// for programs that have such stages or value stages with a guard (also
// without any URI kernel before it).  Re-counts the wave's statuses.
__global__ __launch_bounds__(PW) void k_derived_lines(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                      const DeviceArgs* __restrict__ args) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const int64_t wave = blockIdx.x;
    if (wave * PW >= n_lines || C.meta->cap_ovf) return;
    const WaveLines W = wave_lines(C, wave, n_lines, nbytes);
    // a program without URI, list or pair stages has no regions (arena_base is not written) and no
    // per-wave counts: only the value stages' guard of its tokens runs here (lp_program.h ValStage)
    const bool p2 = P.has_phase2();
    int st = W.active ? (int)C.status[W.li] : -1;
    const bool was_ok = st == ST_OK;
    if (st == ST_OK) {
        const int fmt = P.n_fmt > 1 ? (int)C.fmt_id[W.li] : 0;
        const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + W.s;
        const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
        Arena R{C.arena, 0, 0};
        if (p2) {
            const unsigned long long ab = C.arena_base[W.li];
            const int shard = (int)(ab / C.shard_cap);
            R.p = C.arena + ab;
            R.top = &C.meta->shard_top[16 * shard];
            R.base = ab - (unsigned long long)shard * C.shard_cap;
            R.limit = C.shard_cap;
        }
        st = derived_line(P, fmt, ls - mis, mis, crlf_len_hbm(buf, W), R, C, W.li);
        if (R.ovf) atomicAdd(&C.meta->arena_ovf, 1ull);  // the batch is re-run with a larger arena
        if (st != ST_OK) C.status[W.li] = (uint8_t)st;
    }
    if (!p2) {
        // the batch's counters come from the chunks' counts (launch_parse): move the lines the guard
        // took from OK to their new status (the sums commute with the reduction that follows)
        const unsigned long long bad = __popcll(__ballot(was_ok && st == ST_BAD)),
                                 fb = __popcll(__ballot(was_ok && st == ST_FALLBACK));
        if (lane_id() == 0 && (bad | fb)) {
            atomicAdd(&C.meta->counters[1], 0ull - (bad + fb));
            if (bad) atomicAdd(&C.meta->counters[2], bad);
            if (fb) atomicAdd(&C.meta->counters[3], fb);
        }
        return;
    }
    const uint32_t ok = (uint32_t)__popcll(__ballot(st == ST_OK)), bad = (uint32_t)__popcll(__ballot(st == ST_BAD));
    if (lane_id() == 0) {
        LP_G uint32_t* wc = C.wave_counts + WC_WORDS * (size_t)wave;
        const uint32_t act = wc[0];
        wc[1] = ok;
        wc[2] = bad;
        wc[3] = act - ok - bad;
    }
}

}  // namespace

int launch_uri(const ParseLaunch& a, const DeviceArgs* d_args, hipStream_t s) {
    const int64_t waves = parse_waves(a.cap_lines);
    if (waves == 0 || (!a.uri && !a.derived)) return 0;
    const int64_t grid = waves < 1024 ? waves : 1024;
    // most programs have at most two URI and two query stages (the request
    // URI and the referer): an instance keeping two of each
    if (!a.uri) {
        // (only a token's value-stage guard: k_derived_lines alone)
    } else if (a.n_uri <= 2 && a.n_query <= 2) {
        hipLaunchKernelGGL((k_uri_lines<2, 2>), dim3((unsigned)waves), dim3(PW), 0, s, a.buf, a.nbytes, d_args);
        hipLaunchKernelGGL((k_uri_overflow<2, 2>), dim3((unsigned)grid), dim3(PW), 0, s, a.buf, a.nbytes, d_args);
    } else {
        hipLaunchKernelGGL((k_uri_lines<MAX_URI, MAX_QUERY>), dim3((unsigned)waves), dim3(PW), 0, s, a.buf, a.nbytes,
                           d_args);
        hipLaunchKernelGGL((k_uri_overflow<MAX_URI, MAX_QUERY>), dim3((unsigned)grid), dim3(PW), 0, s, a.buf, a.nbytes,
                           d_args);
    }
    if (a.derived) hipLaunchKernelGGL(k_derived_lines, dim3((unsigned)waves), dim3(PW), 0, s, a.buf, a.nbytes, d_args);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

#if defined(LP_PROFILE)
int prof_read_uri(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * PROF_WAVES * PROF_POINTS) == hipSuccess ? 0 : -1;
}
int prof_clear_uri() {
    static unsigned long long z[PROF_WAVES * PROF_POINTS];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace lp
