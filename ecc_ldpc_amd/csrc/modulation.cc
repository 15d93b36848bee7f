// modulation.cc -- the modulation object of include/ldpc_hip.h (host only): a labelled constellation of 2^m points, m = 1..6, as a
// table, or a product of two level sets of 2^b levels, b = 1..6 (m = 2 b).
// The built-in tables are restated in tests/modulation_spec.py and tests/product_modulation_spec.py, formula for formula.
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

ldpc_modulation *ldpc_modulation_create_product(int bits_per_axis, const float *levels_i, const float *levels_q) {
    if (bits_per_axis < 1 || bits_per_axis > ldpc::kAxisMaxBits || !levels_i || !levels_q) {
        set_error(LDPC_EINVAL, "ldpc_modulation_create_product: bits per axis %d outside 1..%d, or a null table", bits_per_axis, ldpc::kAxisMaxBits);
        return nullptr;
    }
    const int n = 1 << bits_per_axis;
    for (int i = 0; i < n; i++)
        if (!isfinite(levels_i[i]) || !isfinite(levels_q[i])) {
            set_error(LDPC_EINVAL, "ldpc_modulation_create_product: level %d is not finite", i);
            return nullptr;
        }
    ldpc_modulation *mod = new (std::nothrow) ldpc_modulation();
    if (!mod) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    mod->b = bits_per_axis;
    mod->m = 2 * bits_per_axis;
    for (int i = 0; i < n; i++) { mod->ax.lev[0][i] = levels_i[i]; mod->ax.lev[1][i] = levels_q[i]; }
    double acc = 0.0;   // the rule of ldpc_modulation_create on the materialised table, in its index order
    for (int p = 0; p < n * n; p++) {
        const double i = levels_i[p >> bits_per_axis], q = levels_q[p & (n - 1)];
        acc += i * i + q * q;
    }
    mod->es = acc / (double)(n * n);
    return mod;
}

ldpc_modulation *ldpc_modulation_create_builtin(int kind) {
    if (kind == LDPC_MOD_64QAM || kind == LDPC_MOD_256QAM || kind == LDPC_MOD_1024QAM || kind == LDPC_MOD_4096QAM) {
        // square QAM, b = kind / 2 bits an axis: position k has amplitude (2k - (2^b - 1)) / sqrt(2 (4^b - 1) / 3) and carries the label
        // k ^ (k >> 1) (binary-reflected Gray); each level is rounded to float32 once.  Unit energy
        const int b = kind / 2, n = 1 << b;
        float lev[ldpc::kAxisMaxLevels];
        const double norm = sqrt(2.0 * (double)(n * n - 1) / 3.0);
        for (int k = 0; k < n; k++) lev[k ^ (k >> 1)] = (float)((double)(2 * k - (n - 1)) / norm);
        return ldpc_modulation_create_product(b, lev, lev);
    }
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
            set_error(LDPC_EINVAL, "ldpc_modulation_create_builtin: unknown kind %d (LDPC_MOD_BPSK = 1 .. LDPC_MOD_16QAM = 4, LDPC_MOD_64QAM = 6 .. LDPC_MOD_4096QAM = 12)", kind);
            return nullptr;
    }
}

ldpc_modulation *ldpc_modulation_with_rule(const ldpc_modulation *mod, int rule) {
    if (!mod || (rule != LDPC_DEMAP_MAXLOG && rule != LDPC_DEMAP_LOGMAP)) {
        set_error(LDPC_EINVAL, "ldpc_modulation_with_rule: null modulation, or unknown rule %d (LDPC_DEMAP_MAXLOG = 0, LDPC_DEMAP_LOGMAP = 1)", rule);
        return nullptr;
    }
    ldpc_modulation *copy = new (std::nothrow) ldpc_modulation(*mod);
    if (!copy) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    copy->rule = rule;
    return copy;
}

int ldpc_modulation_rule(const ldpc_modulation *mod) { return mod ? mod->rule : set_error(LDPC_EINVAL, "null modulation"); }

void ldpc_modulation_destroy(ldpc_modulation *mod) { delete mod; }

int ldpc_modulation_bits(const ldpc_modulation *mod) { return mod ? mod->m : set_error(LDPC_EINVAL, "null modulation"); }

int ldpc_modulation_points(const ldpc_modulation *mod, float *out) {
    if (!mod) return set_error(LDPC_EINVAL, "null modulation");
    const int n = 1 << mod->m;
    if (mod->b) {   // a product object: the materialised table
        for (int p = 0; out && p < n; p++) { out[2 * p] = mod->ax.lev[0][p >> mod->b]; out[2 * p + 1] = mod->ax.lev[1][p & ((1 << mod->b) - 1)]; }
        return n;
    }
    for (int p = 0; out && p < n; p++) { out[2 * p] = mod->tab.pt[p][0]; out[2 * p + 1] = mod->tab.pt[p][1]; }
    return n;
}

int ldpc_modulation_axis_levels(const ldpc_modulation *mod, float *levels_i, float *levels_q) {
    if (!mod) return set_error(LDPC_EINVAL, "null modulation");
    for (int i = 0; mod->b && i < (1 << mod->b); i++) {
        if (levels_i) levels_i[i] = mod->ax.lev[0][i];
        if (levels_q) levels_q[i] = mod->ax.lev[1][i];
    }
    return mod->b;
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
