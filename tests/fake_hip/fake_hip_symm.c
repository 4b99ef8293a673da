/* fake_hip_symm.c -- TEST INFRASTRUCTURE: the CPU stand-in of fake_hip.c (included unchanged) plus the two entry points of
 * ensemble requests, sayuri_hip_forward_packed_symm / sayuri_hip_submit_packed_symm.  Device sample i is record src[i] taken
 * through board symmetry symm[i] on the host (the rule of include/sayuri_hip.h) and then evaluated by the stand-in's fixed
 * function of a sample's own planes: a reply is a function of (record, symmetry), so tests/test_ensemble_cpu.py can tell
 * for every one of a request's eight results whether it is the right record under the right symmetry. */
#include "fake_hip.c"

static unsigned* symm_records(const sayuri_hip_ctx* c, int n, const unsigned* rec, int n_records, int binary, const int* bsz,
                              const int* src, const int* symm) {
    const int words = binary * 12 + 8;
    if (!symm || n_records <= 0 || (!src && n > n_records)) return NULL;
    for (int i = 0; i < n; ++i)
        if (symm[i] < 0 || symm[i] > 7 || (src && (src[i] < 0 || src[i] >= n_records))) return NULL;
    unsigned* out = (unsigned*)calloc((size_t)n * words, sizeof(unsigned));
    for (int i = 0; i < n; ++i) {
        const unsigned* r = rec + (size_t)(src ? src[i] : i) * words;
        unsigned* o = out + (size_t)i * words;
        const int bs = bsz ? bsz[i] : c->board, s = symm[i];
        memcpy(o + binary * 12, r + binary * 12, 8 * sizeof(unsigned));
        for (int y = 0; y < bs; ++y)
            for (int x = 0; x < bs; ++x) {
                int tx = x, ty = y;
                if (s & 4) { tx = y; ty = x; }
                if (s & 2) tx = bs - 1 - tx;
                if (s & 1) ty = bs - 1 - ty;
                const int d = y * bs + x, q = ty * bs + tx;
                for (int ch = 0; ch < binary; ++ch)
                    if ((r[ch * 12 + (q >> 5)] >> (q & 31)) & 1u) o[ch * 12 + (d >> 5)] |= 1u << (d & 31);
            }
    }
    return out;
}

int sayuri_hip_forward_packed_symm(sayuri_hip_ctx* c, int n, const unsigned* records, int n_records, int binary, const int* bsz,
                                   const int* src, const int* symm, float* prob, float* pass, float* misc, float* own) {
    if (!c || !records || n <= 0 || n > c->max_batch) return -1;
    unsigned* turned = symm_records(c, n, records, n_records, binary, bsz, src, symm);
    if (!turned) return -1;
    const int rc = sayuri_hip_forward_packed(c, n, turned, binary, bsz, prob, pass, misc, own);
    free(turned);
    return rc;
}

int sayuri_hip_submit_packed_symm(sayuri_hip_ctx* c, int n, const unsigned* records, int n_records, int binary, const int* bsz,
                                  const int* src, const int* symm, float* prob, float* pass, float* misc, float* own, int* ticket) {
    if (!c || !records || n <= 0 || n > c->max_batch) return -1;
    unsigned* turned = symm_records(c, n, records, n_records, binary, bsz, src, symm);
    if (!turned) return -1;
    float* x = expand_records(c, n, turned, binary, bsz); /* (the planes are the job's own: also in cheap mode) */
    free(turned);
    const int rc = submit_any(c, n, x, x, bsz, prob, pass, misc, own, ticket);
    if (rc) free(x);
    return rc;
}
