// qm_block.h -- lossy quality values (./harc -c -q -b SPEC; README: "-b and what it promises").  A quality text is n lines of exactly L bytes and a newline; a
// value is a byte v in 33..126 with Phred score q = v - 33; newlines, and bytes outside 33..126, are never changed.  Every rule lives here once: the tables of
// the schemes, the run smoothing of one line, the statistics, the serial mapper that harc_amd_qmap_host runs -- and the bodies of the two kernels of qmap.hip as
// functions of a lane number, so that tests/test_qmap_host.py can run them with the lanes as loops, built by g++ with sanitizers, against the serial mapper.
//
//   a table (ill8, bin:T:H:L, cap:M)   v -> table[v]; valid when it keeps every byte outside 33..126 and maps 33..126 into itself.
//   pblock:R                           a line is cut left to right into blocks: a block starts at the first byte not yet in one, with lo = hi = that byte, and
//                                      takes the next byte v while max(hi, v) - min(lo, v) <= 2 R; every byte of it becomes floor((lo + hi) / 2), so no value
//                                      moves by more than R.  A byte outside 33..126 is a block of its own, unchanged.  Not idempotent.
//
// The table pass (qm_table_item) works in 16-byte chunks of the OUTPUT: the bytes in front of its first 16-byte boundary and behind its last go one by one, a chunk
// is one aligned 16-byte store.  The input of a chunk sits at any alignment: it is cut out of the two aligned 16-byte words around it, the second of which starts
// in front of the input's end -- no load leaves the aligned hull of the input.  In place input and output share their alignment and a lane reads what it writes.
// The stride check rides along: newlines in all, and newlines at the columns L, are counted; n - the second are the stride positions without a newline, the
// first - the second the newlines off the stride.
//
// The run smoothing (qm_tile_load / qm_tile_walk / qm_tile_store, a barrier between them) takes a tile of up to 256 whole lines: the tile's bytes come in through
// aligned 16-byte loads of its hull (bytes of the neighbouring tiles are dropped: in place they may be half written) into rows of an odd number of dwords (lanes that walk
// neighbouring rows at the same column are then on different banks), lane t walks row t with the serial rule of qm_pblock_line, and the tile leaves as the table
// pass's output does: bytes up to the first boundary, aligned 16-byte stores, bytes behind the last.
#pragma once
#include "qv_block.h"
#include "../../include/harc_amd.h"

#define QM_KIND_TABLE 1
#define QM_KIND_PBLOCK 2
#define QM_NVAL 94u                                    // the values 33 .. 126
#define QM_MAXR 46u
#define QM_TILE 256u                                   // lines of a run-smoothing tile = lanes of its workgroup

QV_HD int qm_is_value(uint32_t v) { return v - QV_FIRST < QM_NVAL; }

// ------------------------------------------------------------------------------------------------ the tables
// the first byte value that breaks the table rule, or -1
QV_HD int qm_table_bad(const uint8_t *t)
{
    for (uint32_t v = 0; v < 256u; v++)
        if (qm_is_value(v) ? !qm_is_value(t[v]) : t[v] != v) return (int)v;
    return -1;
}
QV_HD uint32_t qm_ill8(uint32_t q) { return q < 2 ? 0u : q < 10 ? 6u : q < 20 ? 15u : q < 25 ? 22u : q < 30 ? 27u : q < 35 ? 33u : q < 40 ? 37u : 40u; }
// scheme 0: ill8, 1: bin (a = T, b = H, c = L), 2: cap (a = M)
QV_HD void qm_fill_table(uint8_t *t, int scheme, uint32_t a, uint32_t b, uint32_t c)
{
    for (uint32_t v = 0; v < 256u; v++) t[v] = (uint8_t)v;
    for (uint32_t q = 0; q < QM_NVAL; q++) {
        const uint32_t m = scheme == 0 ? qm_ill8(q) : scheme == 1 ? (q >= a ? b : c) : (q < a ? q : a);
        t[QV_FIRST + q] = (uint8_t)(QV_FIRST + m);
    }
}

// ------------------------------------------------------------------------------------------------ the statistics
struct QmAcc { uint64_t changed, sum_abs, sum_sq, in_lo, in_hi, out_lo, out_hi, max_abs; };      // presence masks: bit v - 33, 94 of them
QV_HD void qm_acc_zero(QmAcc *a) { a->changed = a->sum_abs = a->sum_sq = a->in_lo = a->in_hi = a->out_lo = a->out_hi = a->max_abs = 0; }
// v, w in 33..126: a value and what it became
QV_HD void qm_acc_add(QmAcc *a, uint32_t v, uint32_t w)
{
    const uint32_t d = v > w ? v - w : w - v, ki = v - QV_FIRST, ko = w - QV_FIRST;
    a->changed += d != 0; a->sum_abs += d; a->sum_sq += d * d;
    if (d > a->max_abs) a->max_abs = d;
    if (ki < 64u) a->in_lo |= 1ull << ki; else a->in_hi |= 1ull << (ki - 64u);
    if (ko < 64u) a->out_lo |= 1ull << ko; else a->out_hi |= 1ull << (ko - 64u);
}
QV_HD void qm_acc_merge(QmAcc *a, const QmAcc *b)
{
    a->changed += b->changed; a->sum_abs += b->sum_abs; a->sum_sq += b->sum_sq;
    a->in_lo |= b->in_lo; a->in_hi |= b->in_hi; a->out_lo |= b->out_lo; a->out_hi |= b->out_hi;
    if (b->max_abs > a->max_abs) a->max_abs = b->max_abs;
}
QV_HD void qm_acc_stats(const QmAcc *a, uint64_t values, harc_amd_qmap_stats *st)
{
    st->values = values; st->changed = a->changed; st->sum_abs = a->sum_abs; st->sum_sq = a->sum_sq; st->max_abs = (uint32_t)a->max_abs;
    st->distinct_in = (uint32_t)(__builtin_popcountll(a->in_lo) + __builtin_popcountll(a->in_hi));
    st->distinct_out = (uint32_t)(__builtin_popcountll(a->out_lo) + __builtin_popcountll(a->out_hi));
    st->reserved = 0;
}

// ------------------------------------------------------------------------------------------------ one line
// in == out (in place) or disjoint.  *nl: newlines among the L bytes
template <bool STATS> QV_HD void qm_table_line(const uint8_t *in, uint8_t *out, uint32_t L, const uint8_t *table, QmAcc *acc, uint64_t *nl)
{
    for (uint32_t j = 0; j < L; j++) {
        const uint32_t v = in[j], w = table[v];
        *nl += v == '\n';
        if (STATS && qm_is_value(v)) qm_acc_add(acc, v, w);
        out[j] = (uint8_t)w;
    }
}
template <bool STATS> QV_HD void qm_pblock_line(const uint8_t *in, uint8_t *out, uint32_t L, uint32_t R, QmAcc *acc, uint64_t *nl)
{
    uint32_t j = 0;
    while (j < L) {
        const uint32_t v0 = in[j];
        if (!qm_is_value(v0)) { *nl += v0 == '\n'; out[j] = (uint8_t)v0; j++; continue; }
        uint32_t lo = v0, hi = v0, e = j + 1;
        while (e < L) {
            const uint32_t v = in[e];
            if (!qm_is_value(v)) break;
            const uint32_t nlo = v < lo ? v : lo, nhi = v > hi ? v : hi;
            if (nhi - nlo > 2u * R) break;
            lo = nlo; hi = nhi; e++;
        }
        const uint32_t mid = (lo + hi) >> 1;
        for (uint32_t k = j; k < e; k++) {                         // (the byte is read before it is written: in place)
            if (STATS) qm_acc_add(acc, in[k], mid);
            out[k] = (uint8_t)mid;
        }
        j = e;
    }
}

// The serial mapper: n lines of L and their newlines, text -> out.  err[0]: stride positions that hold no newline, err[1]: newlines inside a line
template <bool STATS> static inline void qm_map_text(const uint8_t *text, uint64_t n, uint32_t L, const harc_amd_qmap *map, uint8_t *out, QmAcc *acc, uint64_t *err)
{
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *ln = text + i * (L + 1ull); uint8_t *o = out + i * (L + 1ull);
        const uint32_t on = ln[L] == '\n';
        err[0] += !on;
        if (map->kind == QM_KIND_TABLE) {                          // the table pass knows no columns: the byte on the stride goes through the table as well
            uint64_t all = 0;
            qm_table_line<STATS>(ln, o, L + 1u, map->table, acc, &all);
            err[1] += all - on;
        } else {
            qm_pblock_line<STATS>(ln, o, L, (uint32_t)map->radius, acc, &err[1]);
            o[L] = ln[L];
        }
    }
}

// ------------------------------------------------------------------------------------------------ 16 bytes at a time
struct QmV16 { uint64_t q[2]; };
QV_HD QmV16 qm_load16(const uint8_t *p) { QmV16 v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16); return v; }       // p on a 16-byte boundary
QV_HD void qm_store16(uint8_t *p, QmV16 v) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16); }
QV_HD uint64_t qm_funnel(uint64_t lo, uint64_t hi, uint32_t bits) { return bits ? (lo >> bits) | (hi << (64u - bits)) : lo; }
// (both halves are read first: a choice between the two as lvalues is an index into the 16 bytes, which moves them out of registers)
QV_HD uint32_t qm_byte16(const QmV16 &v, uint32_t k) { const uint64_t lo = v.q[0], hi = v.q[1]; return (uint32_t)((k < 8u ? lo : hi) >> (8u * (k & 7u))) & 255u; }
// the 16 bytes at p, p anywhere, p + 16 <= the end of the input: out of the aligned words at p - s and, for s != 0, p - s + 16 < p + 16
QV_HD QmV16 qm_load16_any(const uint8_t *p)
{
    const uint32_t s = (uint32_t)((uintptr_t)p & 15u), bits = 8u * (s & 7u);
    const QmV16 x = qm_load16(p - s);
    if (!s) return x;
    const QmV16 y = qm_load16(p - s + 16);
    QmV16 r;
    if (s < 8u) { r.q[0] = qm_funnel(x.q[0], x.q[1], bits); r.q[1] = qm_funnel(x.q[1], y.q[0], bits); }
    else { r.q[0] = qm_funnel(x.q[1], y.q[0], bits); r.q[1] = qm_funnel(y.q[0], y.q[1], bits); }
    return r;
}
template <bool STATS> QV_HD uint64_t qm_map8(uint64_t x, const uint8_t *table, QmAcc *acc, uint32_t *newlines)
{
    uint64_t y = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t b = (uint32_t)(x >> (8u * k)) & 255u, w = table[b];
        *newlines += b == '\n';
        if (STATS && qm_is_value(b)) qm_acc_add(acc, b, w);
        y |= (uint64_t)w << (8u * k);
    }
    return y;
}
template <bool STATS> QV_HD QmV16 qm_map16(const QmV16 &v, const uint8_t *table, QmAcc *acc, uint64_t *nl)
{
    QmV16 r;
    uint32_t newlines = 0;
    r.q[0] = qm_map8<STATS>(v.q[0], table, acc, &newlines);       // (no loop over the halves: an index into the 16 bytes would move them out of registers)
    r.q[1] = qm_map8<STATS>(v.q[1], table, acc, &newlines);
    *nl += newlines;
    return r;
}

// ------------------------------------------------------------------------------------------------ the table pass, lane g of G over the N = n (L + 1) bytes
// err[0]: newlines at the columns L (on the stride), err[1]: newlines in all
template <bool STATS> QV_HD void qm_table_item(const uint8_t *in, uint8_t *out, uint64_t N, uint32_t L, const uint8_t *table, uint64_t g, uint64_t G, QmAcc *acc, uint64_t *err)
{
    const uint32_t LL = L + 1u;
    const uint64_t head0 = (uint64_t)((0 - (uintptr_t)out) & 15u), head = head0 < N ? head0 : N, nch = (N - head) >> 4, tail = N - head - (nch << 4);
    uint64_t on = 0, all = 0;                                      // counted in registers, added to err[] on the way out
    for (uint32_t part = 0; part < 2u; part++) {                  // the bytes in front of the first chunk and behind the last
        const uint64_t i = part ? head + (nch << 4) + g : g;
        if (g >= (part ? tail : head)) continue;
        const uint32_t v = in[i], w = table[v];
        if (v == '\n') { all++; on += i % LL == L; }
        if (STATS && qm_is_value(v)) qm_acc_add(acc, v, w);
        out[i] = (uint8_t)w;
    }
    uint32_t col = (uint32_t)((head + (g << 4)) % LL);             // the column of the chunk's first byte
    const uint32_t step = (uint32_t)((G << 4) % LL);
    for (uint64_t c = g; c < nch; c += G) {
        const uint64_t at = head + (c << 4);
        const QmV16 v = qm_load16_any(in + at);
        for (uint32_t k = L - col; k < 16u; k += LL) on += qm_byte16(v, k) == '\n';
        qm_store16(out + at, qm_map16<STATS>(v, table, acc, &all));
        col += step; if (col >= LL) col -= LL;
    }
    err[0] += on; err[1] += all;
}

// ------------------------------------------------------------------------------------------------ run smoothing, a tile of m <= 256 lines: T = m (L + 1) bytes
QV_HD uint32_t qm_pitch(uint32_t L) { return ((L + 4u) >> 2) | 1u; }      // dwords of a row that holds L + 1 bytes: an odd number
// src: the tile's first byte in the input -> rows (pitch bytes each), by lane `lane` of `nl`
QV_HD void qm_tile_load(const uint8_t *src, uint32_t T, uint32_t LL, uint32_t pitch, uint8_t *rows, uint32_t lane, uint32_t nl)
{
    const uint32_t s = (uint32_t)((uintptr_t)src & 15u), nch = (s + T + 15u) >> 4;
    for (uint32_t c = lane; c < nch; c += nl) {
        const QmV16 v = qm_load16(src - s + 16u * c);
        const int32_t i0 = (int32_t)(16u * c) - (int32_t)s;       // the tile offset of the chunk's first byte: negative in the first chunk
        const uint32_t first = i0 < 0 ? 0u : (uint32_t)i0;
        uint32_t row = first / LL, col = first - row * LL;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 16u; k++) {
            if ((uint32_t)(i0 + (int32_t)k) >= T) continue;       // in front of the tile (as unsigned: far behind it) or behind it
            rows[row * pitch + col] = (uint8_t)qm_byte16(v, k);
            if (++col == LL) { col = 0; row++; }
        }
    }
}
// lane t < m walks row t.  err[0]: stride positions without a newline, err[1]: newlines inside a line
template <bool STATS> QV_HD void qm_tile_walk(uint8_t *rows, uint32_t m, uint32_t L, uint32_t pitch, uint32_t R, uint32_t t, QmAcc *acc, uint64_t *err)
{
    if (t >= m) return;
    uint8_t *row = rows + t * pitch;
    qm_pblock_line<STATS>(row, row, L, R, acc, &err[1]);
    err[0] += row[L] != '\n';
}
// rows -> dst, the tile's first byte in the output: no byte outside dst[0 .. T) is written
QV_HD void qm_tile_store(uint8_t *dst, uint32_t T, uint32_t LL, uint32_t pitch, const uint8_t *rows, uint32_t lane, uint32_t nl)
{
    const uint32_t head0 = (uint32_t)((0 - (uintptr_t)dst) & 15u), head = head0 < T ? head0 : T, nch = (T - head) >> 4, tail = T - head - (nch << 4);
    for (uint32_t part = 0; part < 2u; part++) {
        const uint32_t i = part ? head + (nch << 4) + lane : lane;
        if (lane >= (part ? tail : head)) continue;
        const uint32_t row = i / LL;
        dst[i] = rows[row * pitch + (i - row * LL)];
    }
    for (uint32_t c = lane; c < nch; c += nl) {
        const uint32_t at = head + (c << 4);
        uint32_t row = at / LL, col = at - row * LL;
        uint64_t y[2] = { 0, 0 };
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 16u; k++) {
            y[k >> 3] |= (uint64_t)rows[row * pitch + col] << (8u * (k & 7u));
            if (++col == LL) { col = 0; row++; }
        }
        QmV16 v; v.q[0] = y[0]; v.q[1] = y[1];
        qm_store16(dst + at, v);
    }
}
