// Host build of csrc/parse_float.h for the CPU tests (test infrastructure only): the cell parsers are
// device code in the library; here `__device__` is defined away so the same source runs on the host
// against Python's float(), int() and datetime.date (tests/test_csv_scan.py).
#define __device__
#include "parse_float.h"

namespace {
struct HostSrc {
    const unsigned char *p;
    unsigned char at(long long i) const { return p[i]; }
};
}  // namespace

// 0: *bits is the double; 1: cannot decide; 2: not in the grammar
extern "C" int parse_f64_c(const char *s, long long n, unsigned long long *bits) {
    HostSrc src{(const unsigned char *)s};
    uint64_t b = 0;
    const int r = qeh::parse_f64_text(src, 0, n, &b);
    *bits = b;
    return r;
}
extern "C" int parse_int_c(const char *s, long long n, unsigned long long max, long long *out) {
    HostSrc src{(const unsigned char *)s};
    int64_t v = 0;
    const int r = qeh::parse_int_text(src, 0, n, max, &v);
    *out = v;
    return r;
}
extern "C" int parse_date32_c(const char *s, long long n, int *out) {
    HostSrc src{(const unsigned char *)s};
    int32_t v = 0;
    const int r = qeh::parse_date32_text(src, 0, n, &v);
    *out = v;
    return r;
}
