// GlsBatchIn::check (periodicity_amd/csrc/pdc_internal.h) on its own, for a host build under
// -fsanitize=address,undefined: the good and bad `offsets` of tests/test_host_entry_errors.py, the status, the text
// and the sizes it fills.  It makes no HIP call, so this program needs no device (and links no library of ours).
//   hipcc -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -std=c++17 gls_batch_offsets_check.cpp -o check
#include <cstring>
#include <vector>

#include "../../periodicity_amd/csrc/pdc_internal.h"

static char g_text[512];
void pdc::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof(g_text), fmt, ap);
    va_end(ap);
}

static int failures = 0;
static void expect(const char *what, std::vector<int64_t> offsets, int shared_t, int status, const char *text,
                   int64_t n_total = 0, int64_t n_t = 0, int64_t n_max = 0) {
    offsets.shrink_to_fit();   // (the sanitizer's red zone starts right behind offsets[n_curves])
    g_text[0] = 0;
    pdc::GlsBatchIn in;
    const int got = in.check(what, offsets.data(), (int64_t)offsets.size() - 1, shared_t);
    const bool sizes = status != PDC_OK || (in.n_total == n_total && in.n_t == n_t && in.n_max == n_max);
    if (got != status || strcmp(g_text, text) != 0 || !sizes) {
        ++failures;
        printf("FAILED %s shared_t=%d: status %d (want %d), text \"%s\" (want \"%s\"), sizes %lld %lld %lld\n", what, shared_t,
               got, status, g_text, text, (long long)in.n_total, (long long)in.n_t, (long long)in.n_max);
    }
}

int main() {
    for (const char *what : {"gls", "gls_fft_batch"}) {
        const std::string w(what);
        expect(what, {0, 5, 8}, 0, PDC_OK, "", 8, 8, 5);
        expect(what, {0, 4, 8}, 1, PDC_OK, "", 8, 4, 4);
        expect(what, {0, 8}, 0, PDC_OK, "", 8, 8, 8);
        expect(what, {0, 0, 3, 3}, 0, PDC_OK, "", 3, 3, 3);
        expect(what, {0, 0}, 1, PDC_OK, "", 0, 0, 0);
        expect(what, {0, 5, 3}, 0, PDC_ERR_INVALID, (w + ": offsets must be non-decreasing").c_str());
        expect(what, {0, 5, 8}, 1, PDC_ERR_INVALID, (w + ": with a shared time axis every curve must have the same length").c_str());
        expect(what, {1, 5, 8}, 0, PDC_ERR_INVALID, (w + ": offsets[0] must be 0").c_str());
        expect(what, {1, 5, 3}, 0, PDC_ERR_INVALID, (w + ": offsets must be non-decreasing").c_str());
        expect(what, {2, 4, 6}, 1, PDC_ERR_INVALID, (w + ": offsets[0] must be 0").c_str());
    }
    printf("gls_batch_offsets_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
