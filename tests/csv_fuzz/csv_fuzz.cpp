// csv_fuzz IN OUT: the csv body of a table of doubles, formatted by xh_dtoa.h on the host exactly as the device kernels
// (xh_csv.hip) lay it out: a line is str(first_id + r) + ',' + ','.join(fields) + '\n'.
//
// IN:  int64 ncols, int64 first_id, then nrows * ncols raw doubles (native byte order), row-major.
// OUT: the text.  Each field is formatted into a buffer of exactly xh_dtoa_len bytes, so that AddressSanitizer sees a
//      field that is longer than announced; 24 bytes is checked as the upper bound of every field.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "xh_dtoa.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: csv_fuzz IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    if (!in) {
        perror(argv[1]);
        return 2;
    }
    int64_t head[2];
    if (fread(head, sizeof(int64_t), 2, in) != 2 || head[0] <= 0 || head[1] < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int64_t ncols = head[0], first_id = head[1];
    std::vector<double> vals;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(double), 4096, in)) > 0) vals.insert(vals.end(), buf, buf + got);
    fclose(in);
    if (vals.size() % (size_t)ncols != 0) {
        fprintf(stderr, "%zu values are no multiple of %lld columns\n", vals.size(), (long long)ncols);
        return 2;
    }
    const int64_t nrows = (int64_t)(vals.size() / (size_t)ncols);
    const uint64_t *pow10 = xh_dtoa_host_table();
    std::string text;
    for (int64_t r = 0; r < nrows; ++r) {
        char id[24];
        text.append(id, (size_t)xh_dtoa_id_put((uint64_t)(first_id + r), id));
        for (int64_t c = 0; c < ncols; ++c) {
            const xh_repr rep = xh_dtoa_repr(vals[(size_t)(r * ncols + c)], pow10);
            const int len = xh_dtoa_len(rep);
            if (len < 0 || len > XH_DTOA_MAX_LEN) {
                fprintf(stderr, "field of %d characters\n", len);
                return 1;
            }
            std::vector<char> field((size_t)len);      // exactly as long as announced
            if (xh_dtoa_put(rep, field.data()) != len) {
                fprintf(stderr, "xh_dtoa_put and xh_dtoa_len disagree\n");
                return 1;
            }
            text.push_back(',');
            text.append(field.data(), (size_t)len);
        }
        text.push_back('\n');
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) {
        perror(argv[2]);
        return 2;
    }
    const bool ok = fwrite(text.data(), 1, text.size(), out) == text.size();
    return (fclose(out) == 0 && ok) ? 0 : 2;
}
