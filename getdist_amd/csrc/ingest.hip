// Chain ingestion (chains.py:115-125 loadNumpyTxt = np.loadtxt): whitespace-separated decimal text resident on the device
// -> fp64 columns, every value the double np.loadtxt gives bit for bit (parsedouble.hpp).  The inverse of export.hip.
//
// The text is row-major with lines of varying length, the samples are column-major, so the work is tiled over BYTES: seen
// from the 16-byte boundary at or below its first byte the text is cut into tiles of ING_TB bytes, and a block owns the
// lines that START in its tile.  It stages ING_WIN = ING_TB + GD_PARSE_MAX_LINE bytes through LDS (aligned 16-byte loads,
// lanes on consecutive addresses), so every owned line of at most GD_PARSE_MAX_LINE bytes is there to its end; a longer
// one makes the text "not plain".
// Thread t then owns the 128-byte span t of the staged bytes (the LDS image is padded by one word per span: the lanes of
// a wave read words 33 apart, on different banks):
//   walk 1  runs the line state machine (comment / inside a token / tokens so far in the line) over its span from a
//           neutral state and leaves a summary: newlines, tokens before the first and after the last one, data rows
//           strictly inside;
//   compose every thread chains the summaries from the nearest newline before its span: the true state at the span's
//           start and whether the tile owns that line; a prefix sum over the block numbers the rows; the thread of the
//           last span settles the tile's row count and the unfinished last line;
//   walk 2  runs the machine again from the true state.  A lane that meets the first byte of a token knows its row and
//           field and NOTES the token: the lanes of a wave meet theirs at different bytes, and converting it there would
//           run the conversion once per byte of the span instead of once per token;
//   take    one token per lane: its end is found and the scan kernel checks the grammar, the parse kernel converts it.
// The parse kernel notes token (row, field) in slot row * m + field of an LDS block, converts in place and stores the block
// with lanes running along rows, so each column receives consecutive 8-byte stores (a tile of 52-field "%.8e" rows holds
// about 31 of them); a tile with more than ING_VCAP values (very short tokens) converts and stores each value where the
// walk meets it.  Rows are numbered across tiles by the scan of
// the per-tile row counts (tilescan.hpp), as the export's byte counts are.
#include "ctx.hpp"
#include "parsedouble.hpp"
#include "tilescan.hpp"

#define ING_THREADS 256
#define ING_SPAN 128
#define ING_TB 24576                      // bytes whose line starts a tile owns: 192 spans
#define ING_WIN (ING_THREADS * ING_SPAN)  // bytes staged: 32768
static_assert(ING_WIN - ING_TB == GD_PARSE_MAX_LINE, "the documented line limit is the staged overhang");
#define ING_OWN_SPANS (ING_TB / ING_SPAN)
// (both sized so that three blocks share the 160 KB of a CU)
#define ING_VCAP 1792  // values a tile collects in LDS before storing them column by column
#define ING_SCAP 6144  // tokens a tile of the scan notes before checking them one per lane
#define ING_NO_TOKEN 0xffffffffffffffffULL
#define ING_TXT_LDS (ING_WIN + ING_THREADS * 4)
#define ING_SPANS_LDS (ING_TXT_LDS + ING_THREADS * 8)
#define ING_SCAN_LDS (ING_SPANS_LDS + ING_SCAP * 2)
#define ING_PARSE_LDS (ING_SPANS_LDS + ING_VCAP * 8)
static_assert(ING_PARSE_LDS <= 65536 && ING_SCAN_LDS <= 65536, "dynamic LDS within 64 KB");

// why a text is not plain (ParseRes::flags)
#define ING_BAD_BYTE 1
#define ING_RAGGED 2
#define ING_LONG_LINE 4
#define ING_NOT_NUMBER 8

struct ParseRes {
    int flags;
    int m;                    // fields per row: the first count any tile saw
    long long consumed;       // start of the unfinished last line, or nbytes
    unsigned long long nfix;  // undecided tokens (counted past the list's capacity)
};

struct ParseArgs {
    const unsigned char* text;
    int64_t nbytes;
    int phase0;  // text - phase0 is a multiple of 16
    int last;    // the text ends the file: a final line without '\n' counts
    int m;       // 0 in the scan (unknown), the row width in the parse
    // parse only
    double* out;
    int64_t ld, row_offset, rows;
    int64_t* fix;
    int64_t fix_capacity;
};

struct SpanSummary {  // walk 1
    unsigned char nl, first_nl, last_nl, head_tok, tail_tok, inner_rows, flags, pad;
};
#define SS_HEAD_HASH 1
#define SS_TAIL_HASH 2
#define SS_FIRST_OTHER 4
#define SS_ENDS_TOK 8

enum { C_OTHER = 0, C_SEP, C_NL, C_HASH, C_BAD, C_CR };

__device__ __forceinline__ int ing_class(int c) {
    if (c == '\n') return C_NL;
    if (c == '#') return C_HASH;
    if (c == ' ' || c == '\t' || c == 0x0b || c == 0x0c) return C_SEP;
    if (c == '\r') return C_CR;
    if (c == 0 || c >= 0x80) return C_BAD;
    return C_OTHER;
}

__device__ __forceinline__ int ing_pad(int P) { return P + ((P >> 7) << 2); }

struct LdsGet {
    const unsigned char* txt;
    int P0;
    __device__ int operator()(int i) const { return txt[ing_pad(P0 + i)]; }
};

// The tile's bytes: local position P <-> global byte  tile * ING_TB + P - phase0  of the text; [lo, hi) are there.
struct Tile {
    int lo, hi;
    int at_end;       // the staged window reaches the end of the text
    int64_t origin;   // text offset of P = 0 (negative inside tile 0 when phase0 > 0)
};

__device__ __forceinline__ Tile ing_tile(const ParseArgs& p) {
    Tile t;
    t.origin = (int64_t)blockIdx.x * ING_TB - p.phase0;
    t.lo = blockIdx.x == 0 ? p.phase0 : 0;
    const int64_t left = p.nbytes - t.origin;
    t.hi = left < ING_WIN ? (int)left : ING_WIN;
    t.at_end = left <= ING_WIN;
    return t;
}

__device__ __forceinline__ void ing_stage(const ParseArgs& p, const Tile& t, unsigned char* txt) {
    for (int c = threadIdx.x; c * 16 < t.hi; c += ING_THREADS) {
        const int P = c * 16;
        if (P + 16 <= t.lo) continue;
        const unsigned char* g = p.text + (t.origin + P);  // 16-byte aligned by the choice of origin
        if (P >= t.lo && P + 16 <= t.hi) {
            const uint4 v = *(const uint4*)g;
            unsigned int* d = (unsigned int*)(txt + ing_pad(P));
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
            for (int i = 0; i < 16; ++i)
                if (P + i >= t.lo && P + i < t.hi) txt[ing_pad(P + i)] = g[i];
        }
    }
}

// class of the byte at P with '\r' resolved: a separator directly before '\n', otherwise not plain.  As the last byte of
// a text that goes on (not `last`) it belongs to the unfinished line, which is not consumed.
__device__ __forceinline__ int ing_class_at(const ParseArgs& p, const Tile& t, const unsigned char* txt, int P, int c) {
    int k = ing_class(c);
    if (k == C_CR) {
        if (P + 1 < t.hi)
            k = txt[ing_pad(P + 1)] == '\n' ? C_SEP : C_BAD;
        else
            k = (t.at_end && p.last) ? C_BAD : C_SEP;
    }
    return k;
}

template <bool PARSE>
static __global__ void __launch_bounds__(ING_THREADS) k_ingest(ParseArgs p, long long* __restrict__ tile_rows,
                                                               ParseRes* __restrict__ res) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* txt = smem;
    SpanSummary* sum = (SpanSummary*)(smem + ING_TXT_LDS);
    unsigned long long* slots = (unsigned long long*)(smem + ING_SPANS_LDS);  // parse: a noted token, then its value
    unsigned short* list = (unsigned short*)(smem + ING_SPANS_LDS);           // scan: the noted tokens
    __shared__ int s_flags, s_m, s_rows, s_skip, s_ntok, s_own0, s_wave_rows[ING_THREADS / WAVE];

    const Tile t = ing_tile(p);
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_flags = 0, s_m = p.m, s_rows = 0, s_skip = ING_WIN, s_ntok = 0;
        s_own0 = blockIdx.x == 0 || p.text[t.origin - 1] == '\n';
    }
    ing_stage(p, t, txt);
    __syncthreads();

    const int a = tid * ING_SPAN > t.lo ? tid * ING_SPAN : t.lo;
    const int b = (tid + 1) * ING_SPAN < t.hi ? (tid + 1) * ING_SPAN : t.hi;

    // f(P, byte) for the bytes of this thread's span, read a word at a time
    auto for_bytes = [&](auto&& f) {
        const int base = tid * ING_SPAN;
        const unsigned int* words = (const unsigned int*)(txt + ing_pad(base));
        for (int wi = (a - base) >> 2; wi < ((b - base + 3) >> 2); ++wi) {
            const unsigned int word = words[wi];
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                const int P = base + wi * 4 + bi;
                if (P >= a && P < b) f(P, (int)((word >> (8 * bi)) & 255u));
            }
        }
    };

    {  // walk 1: from the neutral state
        SpanSummary s = {};
        int cm = 0, tk = 0, cur = 0, flags = 0;
        for_bytes([&](int P, int c) {
            const int k = ing_class_at(p, t, txt, P, c);
            if (k == C_NL) {
                if (s.nl == 0) {
                    s.head_tok = (unsigned char)cur;
                    flags |= cm ? SS_HEAD_HASH : 0;
                    s.first_nl = (unsigned char)(P & (ING_SPAN - 1));
                } else if (cur > 0) {
                    ++s.inner_rows;
                }
                ++s.nl;
                s.last_nl = (unsigned char)(P & (ING_SPAN - 1));
                cur = 0, cm = 0, tk = 0;
            } else if (k == C_HASH) {
                cm = 1, tk = 0;
            } else if (k == C_OTHER) {
                if (P == a) flags |= SS_FIRST_OTHER;
                if (!cm && !tk) ++cur, tk = 1;
            } else {
                tk = 0;
                if (k == C_BAD && P < ING_TB) atomicOr(&s_flags, ING_BAD_BYTE);
            }
        });
        if (s.nl == 0) {
            s.head_tok = (unsigned char)cur;
            flags |= cm ? SS_HEAD_HASH : 0;
        } else {
            s.tail_tok = (unsigned char)cur;
            flags |= cm ? SS_TAIL_HASH : 0;
        }
        flags |= tk ? SS_ENDS_TOK : 0;
        s.flags = (unsigned char)flags;
        sum[tid] = s;
    }
    __syncthreads();

    // compose: the true state at the start of this thread's span.  The machine forgets everything at a newline, so the
    // thread walks back to the nearest span that holds one (a few spans for chain rows, at most the tile) and chains
    // the summaries from there; the rows finished inside each span are then numbered by a prefix sum over the block.
    const int ns = (t.hi + ING_SPAN - 1) / ING_SPAN;
    int c_cm = 0, c_tk = 0, c_toks = 0, c_own = 0, c_row = 0;
    {
        int line_start = t.lo, add = 0;
        auto chain = [&](const SpanSummary& u) {  // over a span without a newline
            if (!c_cm) {
                c_toks += u.head_tok - ((c_tk && (u.flags & SS_FIRST_OTHER)) ? 1 : 0);
                c_cm = (u.flags & SS_HEAD_HASH) != 0;
                c_tk = (u.flags & SS_ENDS_TOK) != 0;
            }
        };
        auto restart = [&](const SpanSummary& u, int span) {  // behind the last newline of a span
            line_start = span * ING_SPAN + u.last_nl + 1;
            c_own = line_start < ING_TB;
            c_toks = u.tail_tok;
            c_cm = (u.flags & SS_TAIL_HASH) != 0;
            c_tk = (u.flags & SS_ENDS_TOK) != 0;
        };
        if (tid < ns) {
            int j = tid - 1;
            while (j >= 0 && sum[j].nl == 0) --j;
            if (j >= 0)
                restart(sum[j], j);
            else
                c_own = s_own0;  // a line starts at the tile's first byte
            for (int i = j + 1; i < tid; ++i) chain(sum[i]);
            const SpanSummary u = sum[tid];
            if (u.nl) {
                const int head = c_cm ? 0 : u.head_tok - ((c_tk && (u.flags & SS_FIRST_OTHER)) ? 1 : 0);
                if (c_own && c_toks + head > 0) add = 1;
                if (c_own && tid * ING_SPAN + u.first_nl + 1 - line_start > GD_PARSE_MAX_LINE) atomicOr(&s_flags, ING_LONG_LINE);
                if (tid < ING_OWN_SPANS) add += u.inner_rows;
            }
        }
        int incl = add;  // inclusive scan: the wave, then the four waves
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if ((tid & (WAVE - 1)) >= o) incl += v;
        }
        if ((tid & (WAVE - 1)) == WAVE - 1) s_wave_rows[tid / WAVE] = incl;
        __syncthreads();
        for (int w = 0; w < tid / WAVE; ++w) incl += s_wave_rows[w];
        c_row = incl - add;
        if (tid == ns - 1) {  // the state behind the last staged byte, and what becomes of an unfinished last line
            int row = incl, cm = c_cm, tk = c_tk, toks = c_toks, own = c_own;
            const SpanSummary u = sum[tid];
            if (u.nl) {
                restart(u, tid);
            } else {
                chain(u);
            }
            if (c_own && line_start < t.hi) {  // the tile's last line has no '\n' among the staged bytes
                if (!t.at_end || t.hi - line_start > GD_PARSE_MAX_LINE) {
                    atomicOr(&s_flags, ING_LONG_LINE);
                } else if (p.last) {
                    if (c_toks > 0) {
                        ++row;
                        const int seen = p.m ? p.m : atomicCAS(&s_m, 0, c_toks);
                        if (seen != 0 && seen != c_toks) atomicOr(&s_flags, ING_RAGGED);
                    }
                } else {
                    s_skip = line_start;
                    atomicMin(&res->consumed, (long long)(t.origin + line_start));
                }
            }
            s_rows = row;
            c_cm = cm, c_tk = tk, c_toks = toks, c_own = own;  // back to the state at the span's start for walk 2
        }
    }
    __syncthreads();

    const int RT = s_rows;
    const int skip = s_skip;
    // a tile whose values fit the LDS block parses them in place there; a tile with more (very short tokens) takes every
    // token where the walk meets it and stores it directly
    const bool staged = PARSE && (int64_t)RT * p.m <= ING_VCAP;
    const long long row_base = PARSE ? tile_rows[blockIdx.x] : 0;
    if constexpr (PARSE) {
        if (staged)
            for (int i = tid; i < RT * p.m; i += ING_THREADS) slots[i] = ING_NO_TOKEN;
        __syncthreads();
    }

    // One token, first byte at P: the scan checks its grammar; the parse converts it, lists it when undecided, and leaves
    // the bits in *slot or, without a slot, in the output block.
    auto take = [&](int P, int row, int field, unsigned long long* slot) {
        int e = P + 1;
        while (e < t.hi && ing_class(txt[ing_pad(e)]) == C_OTHER) ++e;
        if constexpr (!PARSE) {
            if (gdparse::parse_token_with<false>(LdsGet{txt, P}, e - P, nullptr) != GD_PARSE_DECIDED)
                atomicOr(&s_flags, ING_NOT_NUMBER);
        } else {
            uint64_t bits = 0;
            const int v = gdparse::parse_token_with<true>(LdsGet{txt, P}, e - P, &bits);
            if (v == GD_PARSE_NAN_TOKEN) atomicOr(&s_flags, ING_NOT_NUMBER);
            if (v != GD_PARSE_DECIDED) bits = 0x7ff8000000000000ULL;
            if (v == GD_PARSE_UNDECIDED) {
                const unsigned long long at = atomicAdd(&res->nfix, 1ULL);
                if ((long long)at < p.fix_capacity) {
                    int64_t* f = p.fix + 4 * at;
                    f[0] = p.row_offset + row_base + row;
                    f[1] = field;
                    f[2] = t.origin + P;
                    f[3] = e - P;
                }
            }
            if (slot)
                *slot = bits;
            else
                p.out[(int64_t)field * p.ld + p.row_offset + row_base + row] = __longlong_as_double((long long)bits);
        }
    };

    {  // walk 2: from the true state.  The lanes meet their tokens at different bytes, so a token is only NOTED here (its
       // first byte: in slot row * m + field of the value block in the parse, at the end of a list in the scan) ...
        int cm = c_cm, tk = c_tk, toks = c_toks, row = c_row, own = c_own;
        for_bytes([&](int P, int c) {
            const int k = ing_class_at(p, t, txt, P, c);
            if (k == C_NL) {
                if (own && toks > 0) {
                    const int seen = p.m ? p.m : atomicCAS(&s_m, 0, toks);
                    if (seen != 0 && seen != toks) atomicOr(&s_flags, ING_RAGGED);
                    ++row;
                }
                toks = 0, cm = 0, tk = 0;
                own = P + 1 < ING_TB;
            } else if (k == C_HASH) {
                cm = 1, tk = 0;
            } else if (k != C_OTHER) {
                tk = 0;
            } else if (!cm && !tk) {
                const int field = toks;
                ++toks, tk = 1;
                if (!own || P >= skip) return;
                if constexpr (!PARSE) {
                    const int at = atomicAdd(&s_ntok, 1);
                    if (at < ING_SCAP)
                        list[at] = (unsigned short)P;
                    else
                        take(P, 0, 0, nullptr);
                } else {
                    if (field >= p.m || row >= RT || row_base + row >= p.rows)
                        atomicOr(&s_flags, ING_RAGGED);
                    else if (staged)
                        slots[row * p.m + field] = (unsigned long long)P;
                    else
                        take(P, row, field, nullptr);
                }
            }
        });
    }
    __syncthreads();

    // ... and taken here, one token per lane
    if constexpr (!PARSE) {
        const int n = s_ntok < ING_SCAP ? s_ntok : ING_SCAP;
        for (int i = tid; i < n; i += ING_THREADS) take(list[i], 0, 0, nullptr);
    } else if (staged) {
        const int total = RT * p.m;
        for (int i = tid; i < total; i += ING_THREADS) {
            const unsigned long long P = slots[i];
            if (P == ING_NO_TOKEN) {  // a row short of a field: cannot happen after a clean scan
                atomicOr(&s_flags, ING_RAGGED);
                slots[i] = 0x7ff8000000000000ULL;
            } else {
                take((int)P, i / p.m, i % p.m, &slots[i]);
            }
        }
        __syncthreads();
        for (int i = tid; i < total; i += ING_THREADS) {  // lanes run along rows: consecutive 8-byte stores into every column
            const int f = i / RT, r = i - f * RT;
            if (row_base + r < p.rows)
                p.out[(int64_t)f * p.ld + p.row_offset + row_base + r] = __longlong_as_double((long long)slots[r * p.m + f]);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if constexpr (!PARSE) {
            tile_rows[blockIdx.x] = RT;
            if (s_m > 0) {
                const int seen = atomicCAS(&res->m, 0, s_m);
                if (seen != 0 && seen != s_m) s_flags |= ING_RAGGED;
            }
        }
        if (s_flags) atomicOr(&res->flags, s_flags);
    }
}

static __global__ void k_ingest_init(ParseRes* res, long long nbytes) {
    res->flags = 0, res->m = 0, res->consumed = nbytes, res->nfix = 0;
}

static const char* why_not_plain(int flags) {
    if (flags & ING_BAD_BYTE) return "a NUL, a byte >= 0x80 or a '\\r' that is not followed by '\\n'";
    if (flags & ING_LONG_LINE) return "a line longer than GD_PARSE_MAX_LINE bytes";
    if (flags & ING_RAGGED) return "rows with differing numbers of fields";
    return "a token that is not a number";
}

struct ScanOut {
    long long rows;
    ParseRes res;
    long long* cnt;  // device: exclusive scan of the per-tile row counts
    ParseRes* d_res;
    int nb;
};

// the scan pass of both entry points; blocks until its results are on the host
static int scan_common(gd_ctx* ctx, ParseArgs& p, ScanOut* o) {
    p.phase0 = (int)((uintptr_t)p.text & 15);
    const int64_t nb64 = (p.phase0 + p.nbytes + ING_TB - 1) / ING_TB;
    GD_REQUIRE(nb64 < (1LL << 30), "too much text for one call");
    o->nb = (int)nb64;
    ScratchPlan sp;
    auto cnt = sp.tail<long long>((int64_t)o->nb + 1);  // (tail: the result record follows at once)
    auto d_res = sp.tail<ParseRes>(1);
    GD_TRY(sp.get(ctx));
    o->cnt = cnt, o->d_res = d_res;
    k_ingest_init<<<1, 1, 0, ctx->stream>>>(o->d_res, (long long)p.nbytes);
    GD_KERNEL_CHECK();
    ParseArgs q = p;
    q.m = 0;
    k_ingest<false><<<o->nb, ING_THREADS, ING_SCAN_LDS, ctx->stream>>>(q, o->cnt, o->d_res);
    GD_KERNEL_CHECK();
    GD_TRY(gd_tile_offsets(ctx, o->cnt, o->nb, &o->rows));
    GD_TRY(gd_fetch(ctx, &o->res, o->d_res, sizeof(ParseRes)));
    GD_TRY(gd_stream_sync(ctx));
    if (o->res.flags) {
        gd_fail(ctx, GD_PARSE_NOT_PLAIN, "the text is not plain: %s", why_not_plain(o->res.flags));
        return GD_PARSE_NOT_PLAIN;
    }
    return GD_OK;
}

extern "C" {

int gd_parse_scan(gd_ctx* ctx, const void* d_text, int64_t nbytes, int32_t last, int64_t* rows_out, int32_t* fields_out,
                  int64_t* consumed_out) {
    GD_REQUIRE(ctx && rows_out && fields_out && consumed_out, "null argument");
    GD_REQUIRE(nbytes >= 0 && (d_text || nbytes == 0), "bad text block");
    *rows_out = 0, *fields_out = 0, *consumed_out = 0;
    if (nbytes == 0) return GD_OK;
    ParseArgs p = {};
    p.text = (const unsigned char*)d_text, p.nbytes = nbytes, p.last = last != 0;
    ScanOut o;
    GD_TRY(scan_common(ctx, p, &o));
    *rows_out = o.rows, *fields_out = o.res.m, *consumed_out = o.res.consumed;
    return GD_OK;
}

int gd_parse_rows(gd_ctx* ctx, const void* d_text, int64_t nbytes, int32_t last, int64_t rows, int32_t m, void* d_out, int64_t ld,
                  int64_t row_offset, void* d_fix, int64_t fix_capacity, int64_t* fix_count_out) {
    GD_REQUIRE(ctx && fix_count_out, "null argument");
    GD_REQUIRE(nbytes >= 0 && (d_text || nbytes == 0), "bad text block");
    GD_REQUIRE(rows >= 0 && m >= 0 && row_offset >= 0 && fix_capacity >= 0, "negative size");
    GD_REQUIRE(d_out || rows == 0, "null output block");
    GD_REQUIRE(d_fix || fix_capacity == 0, "null fix list");
    GD_REQUIRE(ld >= row_offset + rows, "ld < row_offset + rows");
    *fix_count_out = 0;
    if (nbytes == 0) {
        GD_REQUIRE(rows == 0, "an empty text holds no rows");
        return GD_OK;
    }
    ParseArgs p = {};
    p.text = (const unsigned char*)d_text, p.nbytes = nbytes, p.last = last != 0;
    ScanOut o;
    GD_TRY(scan_common(ctx, p, &o));
    const long long held = p.last ? (long long)nbytes : o.res.consumed;
    if (o.rows != rows || (rows > 0 && o.res.m != m) || held != (long long)nbytes)
        return gd_fail(ctx, GD_ERR_BADARG, "the text holds %lld rows of %d fields in its first %lld bytes, not %lld of %d in %lld", o.rows,
                       o.res.m, held, (long long)rows, (int)m, (long long)nbytes);
    if (rows == 0) return GD_OK;
    p.m = m, p.out = (double*)d_out, p.ld = ld, p.row_offset = row_offset, p.rows = rows;
    p.fix = (int64_t*)d_fix, p.fix_capacity = fix_capacity;
    k_ingest<true><<<o.nb, ING_THREADS, ING_PARSE_LDS, ctx->stream>>>(p, o.cnt, o.d_res);
    GD_KERNEL_CHECK();
    GD_TRY(gd_fetch(ctx, &o.res, o.d_res, sizeof(ParseRes)));
    GD_TRY(gd_stream_sync(ctx));
    *fix_count_out = (int64_t)o.res.nfix;
    if (o.res.flags) {  // cannot happen after a clean scan of the same bytes
        gd_fail(ctx, GD_PARSE_NOT_PLAIN, "the text is not plain: %s", why_not_plain(o.res.flags));
        return GD_PARSE_NOT_PLAIN;
    }
    return GD_OK;
}

}  // extern "C"
