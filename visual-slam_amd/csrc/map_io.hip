// map_io.hip -- the map as text, host only: PLY export of the device map (mo_map_write_ply; utils.create_point_cloud_ply,
// utils.py:72-118) and the float formatter it is built on (mo_format_floats): floats as Python's repr of the double value.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "map_store.h"

static size_t fmt_double(double v, char* o) {
    if (std::isnan(v)) { std::memcpy(o, "nan", 3); return 3; }
    if (std::isinf(v)) { if (v < 0) { std::memcpy(o, "-inf", 4); return 4; } std::memcpy(o, "inf", 3); return 3; }
    char sci[40];
    // shortest round-trip digits in scientific form: [-]d[.ddd]e(+|-)XX
    auto r = std::to_chars(sci, sci + sizeof(sci), v, std::chars_format::scientific);
    const size_t len = (size_t)(r.ptr - sci);
    sci[len] = '\0';
    size_t k = 0;
    const bool neg = sci[0] == '-';
    if (neg) k = 1;
    char dig[24]; int nd = 0;
    size_t e = k;
    for (; e < len && sci[e] != 'e'; e++) if (sci[e] != '.') dig[nd++] = sci[e];
    const int exp10 = std::atoi(sci + e + 1);
    size_t n = 0;
    if (neg) o[n++] = '-';
    if (exp10 < -4 || exp10 >= 16) {
        o[n++] = dig[0];
        if (nd > 1) { o[n++] = '.'; for (int i = 1; i < nd; i++) o[n++] = dig[i]; }
        o[n++] = 'e'; o[n++] = exp10 < 0 ? '-' : '+';
        const int ae = exp10 < 0 ? -exp10 : exp10;
        if (ae < 10) o[n++] = '0';
        char eb[8]; auto er = std::to_chars(eb, eb + 8, ae);
        for (char* q = eb; q < er.ptr; q++) o[n++] = *q;
        return n;
    }
    if (exp10 < 0) {
        o[n++] = '0'; o[n++] = '.';
        for (int i = 0; i < -exp10 - 1; i++) o[n++] = '0';
        for (int i = 0; i < nd; i++) o[n++] = dig[i];
        return n;
    }
    // exp10 in [0, 16): integer part = first exp10 + 1 digits (zero-padded), then the rest or ".0"
    for (int i = 0; i <= exp10; i++) o[n++] = i < nd ? dig[i] : '0';
    o[n++] = '.';
    if (nd > exp10 + 1) for (int i = exp10 + 1; i < nd; i++) o[n++] = dig[i];
    else o[n++] = '0';
    return n;
}

extern "C" int mo_format_floats(const float* v, int64_t n, char* out, size_t cap, size_t* len) {
    if ((!v && n) || !len) return MO_ERR_ARG;
    size_t w = 0;
    char buf[48];
    for (int64_t i = 0; i < n; i++) {
        const size_t k = fmt_double((double)v[i], buf);
        if (out && w + k + 1 <= cap) { std::memcpy(out + w, buf, k); out[w + k] = '\n'; }
        w += k + 1;
    }
    *len = w;
    return out && w > cap ? MO_ERR_CAPACITY : MO_OK;
}

extern "C" int mo_map_write_ply(mo_map* m, const char* path, int min_obs, int64_t* n_written) {
    if (!m) return MO_ERR_ARG;
    mo_ctx* c = m->c;
    if (!path) return mo_fail(c, MO_ERR_ARG, "NULL path");
    MAP_ENTER(m);
    const size_t np = (size_t)m->n_pts;
    std::vector<float> xyz(np * 3);
    std::vector<uint8_t> col(np * 3);
    std::vector<int32_t> off(np + 1);
    const MapPts p = m->P[m->cur].view();
    if (np) {
        HIPCHK(c, hipMemcpyAsync(xyz.data(), p.xyz, np * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(col.data(), p.col, np * 3, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(off.data(), p.off, (np + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    size_t cnt = 0;
    for (size_t i = 0; i < np; i++) cnt += off[i + 1] - off[i] >= min_obs;
    if (n_written) *n_written = (int64_t)cnt;
    if (!cnt) return MO_OK;  // (local_mapper.py:345: nothing to write, no file)
    std::string s;
    s.reserve(200 + cnt * 64);
    s += "ply\nformat ascii 1.0\nelement vertex " + std::to_string(cnt) +
         "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    char buf[48];
    for (size_t i = 0; i < np; i++) {
        if (off[i + 1] - off[i] < min_obs) continue;
        for (int k = 0; k < 3; k++) { s.append(buf, fmt_double((double)xyz[i * 3 + k], buf)); s += ' '; }
        for (int k = 0; k < 3; k++) {
            auto r = std::to_chars(buf, buf + 8, (int)col[i * 3 + k]);
            s.append(buf, (size_t)(r.ptr - buf));
            s += k < 2 ? ' ' : '\n';
        }
    }
    FILE* fp = std::fopen(path, "wb");
    if (!fp) return mo_fail(c, MO_ERR_ARG, std::string("cannot open ") + path);
    const size_t wr = std::fwrite(s.data(), 1, s.size(), fp);
    const int cl = std::fclose(fp);
    if (wr != s.size() || cl != 0) return mo_fail(c, MO_ERR_ARG, std::string("write failed: ") + path);
    return MO_OK;
}
