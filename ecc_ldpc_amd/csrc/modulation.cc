// modulation.cc -- the modulation object of include/ldpc_hip.h (host only): a labelled constellation of 2^m points, m = 1..6.
// The built-in tables are restated in tests/modulation_spec.py, formula for formula.
#include <math.h>

#include <new>

#include "demap.h"

using ldpc::set_error;

extern "C" {

ldpc_modulation *ldpc_modulation_create(int bits_per_symbol, const float *points) {
    if (bits_per_symbol < 1 || bits_per_symbol > ldpc::kModMaxBits || !points) {
        set_error(LDPC_EINVAL, "ldpc_modulation_create: bits per symbol %d outside 1..%d, or a null table", bits_per_symbol, ldpc::kModMaxBits);
        return nullptr;
    }
    const int n = 1 << bits_per_symbol;
    for (int i = 0; i < 2 * n; i++)
        if (!isfinite(points[i])) {
            set_error(LDPC_EINVAL, "ldpc_modulation_create: point %d is not finite", i / 2);
            return nullptr;
        }
    ldpc_modulation *mod = new (std::nothrow) ldpc_modulation();
    if (!mod) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    mod->m = bits_per_symbol;
    double acc = 0.0;
    for (int p = 0; p < n; p++) {
        const double i = points[2 * p], q = points[2 * p + 1];
        mod->tab.pt[p][0] = points[2 * p];
        mod->tab.pt[p][1] = points[2 * p + 1];
        acc += i * i + q * q;
    }
    mod->es = acc / (double)n;
    return mod;
}

ldpc_modulation *ldpc_modulation_create_builtin(int kind) {
    float pt[16][2];
    const float h = (float)sqrt(0.5);
    switch (kind) {
        case LDPC_MOD_BPSK:
            pt[0][0] = -1.f; pt[0][1] = 0.f; pt[1][0] = 1.f; pt[1][1] = 0.f;
            return ldpc_modulation_create(1, &pt[0][0]);
        case LDPC_MOD_QPSK:
            for (int p = 0; p < 4; p++) { pt[p][0] = (float)(2 * (p >> 1) - 1) * h; pt[p][1] = (float)(2 * (p & 1) - 1) * h; }
            return ldpc_modulation_create(2, &pt[0][0]);
        case LDPC_MOD_8PSK: {   // the point at angle k pi / 4 carries the label k ^ (k >> 1): Gray around the circle
            const float ring[8][2] = {{1.f, 0.f}, {h, h}, {0.f, 1.f}, {-h, h}, {-1.f, 0.f}, {-h, -h}, {0.f, -1.f}, {h, -h}};
            for (int k = 0; k < 8; k++) { pt[k ^ (k >> 1)][0] = ring[k][0]; pt[k ^ (k >> 1)][1] = ring[k][1]; }
            return ldpc_modulation_create(3, &pt[0][0]);
        }
        case LDPC_MOD_16QAM: {  // two bits per axis, Gray: 00 01 11 10 -> -3 -1 +1 +3, times 1 / sqrt 10
            const double lev[4] = {-3.0, -1.0, 3.0, 1.0};
            for (int p = 0; p < 16; p++) { pt[p][0] = (float)(lev[p >> 2] / sqrt(10.0)); pt[p][1] = (float)(lev[p & 3] / sqrt(10.0)); }
            return ldpc_modulation_create(4, &pt[0][0]);
        }
        default:
            set_error(LDPC_EINVAL, "ldpc_modulation_create_builtin: unknown kind %d (LDPC_MOD_BPSK = 1 .. LDPC_MOD_16QAM = 4)", kind);
            return nullptr;
    }
}

void ldpc_modulation_destroy(ldpc_modulation *mod) { delete mod; }

int ldpc_modulation_bits(const ldpc_modulation *mod) { return mod ? mod->m : set_error(LDPC_EINVAL, "null modulation"); }

int ldpc_modulation_points(const ldpc_modulation *mod, float *out) {
    if (!mod) return set_error(LDPC_EINVAL, "null modulation");
    const int n = 1 << mod->m;
    for (int p = 0; out && p < n; p++) { out[2 * p] = mod->tab.pt[p][0]; out[2 * p + 1] = mod->tab.pt[p][1]; }
    return n;
}

double ldpc_modulation_energy(const ldpc_modulation *mod) {
    if (!mod) { set_error(LDPC_EINVAL, "null modulation"); return 0.0; }
    return mod->es;
}

int ldpc_modulation_symbols(const ldpc_modulation *mod, int n_tx) {
    if (!mod || n_tx < 0) return set_error(LDPC_EINVAL, "ldpc_modulation_symbols: null modulation or negative n_tx");
    return (n_tx + mod->m - 1) / mod->m;
}

}  // extern "C"
