// ksampler.cpp -- schedules and evaluation plan of the sigma-schedule samplers (ksampler.hpp).  Host only, f64.
//
// A sampler is written in k-space (x_k = x / c, c(sigma) = 1 / sqrt(1 + sigma^2), D = x_k - sigma e) as one linear row per UNet evaluation,
//     x_k' = A x_k + E e + H q_-1 + Z z + Z2 z2,      q = the one thing the kind keeps (D, stage 1's e, or the step's start latent, in k-space units),
// where x_k is the latent the evaluation ran on (at sigma_e) and x_k' lives at sigma_n.  On the VP latent the engine keeps that is
//     cx = c_n A / c_e,  ce = c_n E,  h1 = c_n H,  cz = c_n Z,  cz2 = c_n Z2;      q = qx x + qe e with the k-space weight on x_k divided by c_e.
// euler and dpmpp_2m are written in the alpha form of sdmi_sampler_coefs instead (a = 1 / (1 + sigma^2)): the same numbers, and on schedule 0 -- whose alphas are the
// table's own -- the same bits, so that the two interfaces cannot drift apart.
#include "ksampler.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "error.hpp"

namespace sdmi {

namespace {

[[noreturn]] void bad(const std::string& m) { throw Error(SDMI_ERR_INVALID, m); }

// ln S_j of the model's table, S_j = sigma(a[j])
struct Table {
    std::vector<double> ln_s;
    Table(const float* alphas, int total) : ln_s((size_t)total) {
        for (int j = 0; j < total; ++j) ln_s[(size_t)j] = std::log(sigma((double)alphas[j]));
    }
    static double sigma(double a) { return std::sqrt((1.0 - a) / a); }
    int total() const { return (int)ln_s.size(); }
    double to_t(double s) const {
        const int n = total();
        if (n < 2) return 0.0;
        const double ls = std::log(s);
        // the last j <= n - 2 with ln S_j <= ln s (0 where there is none: w clamps to 0)
        const auto end = ln_s.begin() + (n - 1);
        const auto it = std::upper_bound(ln_s.begin(), end, ls);
        const int low = it == ln_s.begin() ? 0 : (int)(it - ln_s.begin()) - 1;
        const double lo = ln_s[(size_t)low], hi = ln_s[(size_t)low + 1];
        double w = (lo - ls) / (lo - hi);
        w = w < 0.0 ? 0.0 : w > 1.0 ? 1.0 : w;
        return (double)low + w;
    }
};

void check_table(const float* alphas, int total) {
    if (!alphas) bad("ksampler: null alphas_cumprod");
    if (total < 1) bad("ksampler: total must be positive");
    for (int j = 0; j < total; ++j)   // zero terminal SNR: sigma_max = inf, no sigma schedule
        if (alphas[j] == 0.0f) throw Error(SDMI_ERR_UNSUPPORTED, "ksampler: the schedule holds alphas_cumprod = 0 (zero terminal SNR): sigma_max is infinite");
    for (int j = 0; j < total; ++j)
        if (!(alphas[j] > 0.0f && alphas[j] < 1.0f)) bad("ksampler: alphas_cumprod must lie inside (0, 1)");
}

// a point of the schedule: sigma, a = 1 / (1 + sigma^2), om = 1 - a without the cancellation, and the time the UNet is evaluated at
struct Node { double s, a, om, t; };

Node node_of(const Table& tb, double s) {
    if (s <= 0.0) return Node{0.0, 1.0, 0.0, 0.0};
    const double d = 1.0 + s * s;
    return Node{s, 1.0 / d, s * s / d, tb.to_t(s)};
}
Node node_of_table(const float* alphas, int t) {
    const double a = (double)alphas[t];
    return Node{Table::sigma(a), a, 1.0 - a, (double)t};
}

void anc(double s, double s2, double eta, double* down, double* up) {
    const double u = std::min(s2, eta * std::sqrt(s2 * s2 * (s * s - s2 * s2) / (s * s)));
    *up = u;
    *down = std::sqrt(s2 * s2 - u * u);
}

struct Row { double cx = 0, ce = 0, h1 = 0, cz = 0, cz2 = 0, qx = 0, qe = 0; };

// a k-space row (A, E, H, Z, Z2) of an evaluation at e that lands at n, on the VP latent
Row vp_row(const Node& e, const Node& n, double A, double E, double H, double Z, double Z2) {
    const double cn = std::sqrt(n.a), ce = std::sqrt(e.a);
    Row r;
    r.cx = cn * A / ce; r.ce = cn * E; r.h1 = cn * H; r.cz = cn * Z; r.cz2 = cn * Z2;
    return r;
}

// DDIM(eta) on the pair (cur, prev): sdmi_sampler_coefs' kind 0, expression for expression
Row euler_row(const Node& c, const Node& p, double eta) {
    const double sc = std::sqrt(c.a), sn = std::sqrt(c.om), sp = std::sqrt(p.a);
    const double sigma = eta * std::sqrt(p.om / c.om) * std::sqrt(1.0 - c.a / p.a);
    const double dir = std::sqrt(p.om - sigma * sigma);
    Row r;
    r.cx = sp / sc;
    r.ce = dir - sp * sn / sc;
    r.cz = sigma;
    return r;
}

double lambda(const Node& n) { return 0.5 * std::log(n.a / n.om); }

// DPM-Solver++(2M) on the pair (cur, prev), last = the start of the step before (null: none): sdmi_sampler_coefs' kind 1, expression for expression
Row dpmpp_2m_row(const Node& c, const Node& p, const Node* last) {
    const double sc = std::sqrt(c.a), sn = std::sqrt(c.om), sp = std::sqrt(p.a);
    Row r;
    r.qx = 1.0 / sc; r.qe = -sn / sc;
    if (p.a >= 1.0) { r.cx = r.qx; r.ce = r.qe; return r; }
    const double h = lambda(p) - lambda(c);
    const double A = std::sqrt(p.om / c.om), B = -sp * std::expm1(-h);
    double w0 = 1.0, w1 = 0.0;
    if (last) {
        const double rr = (lambda(c) - lambda(*last)) / h;
        w0 = 1.0 + 1.0 / (2.0 * rr);
        w1 = -1.0 / (2.0 * rr);
    }
    r.cx = A + B * w0 * r.qx;
    r.ce = B * w0 * r.qe;
    r.h1 = B * w1;
    return r;
}

}  // namespace

void check_ksampler(const sdmi_ksampler& k, const float* alphas, int total) {
    const bool table = alphas != nullptr || total != 0;   // (a context whose schedule is not loaded yet checks the bounds' range at its first call)
    if (table) check_table(alphas, total);
    if (k.kind < 0 || k.kind > 6) bad("ksampler: kind must be 0 (euler), 1 (dpmpp_2m), 2 (heun), 3 (dpm2), 4 (dpmpp_2s), 5 (dpmpp_sde) or 6 (dpmpp_2m_sde)");
    if (k.schedule < 0 || k.schedule > 3) bad("ksampler: schedule must be 0 (model), 1 (karras), 2 (exponential) or 3 (uniform)");
    if (!(k.eta >= 0.0 && k.eta <= 1.0)) bad("ksampler: eta must satisfy 0 <= eta <= 1");
    if (k.kind >= 1 && k.kind <= 3 && k.eta != 0.0) bad("ksampler: eta must be 0 for dpmpp_2m, heun and dpm2");
    if (!(k.rho >= 0.0) || !std::isfinite(k.rho)) bad("ksampler: rho must be finite and not negative (0 = 7)");
    const double s_lo = table ? Table::sigma((double)alphas[0]) : 0.0, s_hi = table ? Table::sigma((double)alphas[total - 1]) : INFINITY;
    for (const double b : {k.sigma_min, k.sigma_max}) {
        if (!std::isfinite(b) || b < 0.0) bad("ksampler: sigma_min / sigma_max must be finite and not negative (0 = the model's)");
        if (table && b != 0.0 && (b < s_lo || b > s_hi))
            bad("ksampler: sigma_min / sigma_max must lie inside the model's range [" + std::to_string(s_lo) + ", " + std::to_string(s_hi) + "]");
    }
    const double smin = k.sigma_min != 0.0 ? k.sigma_min : s_lo, smax = k.sigma_max != 0.0 ? k.sigma_max : s_hi;
    if (!(smin < smax)) bad("ksampler: sigma_min must be below sigma_max");
}

double sigma_to_t(const float* alphas, int total, double sigma) {
    check_table(alphas, total);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) bad("sigma_to_t: sigma must be positive and finite");
    return Table(alphas, total).to_t(sigma);
}

std::vector<double> ksampler_sigmas(const sdmi_ksampler& k, const float* alphas, int total, size_t n_steps, std::vector<int>* ts_out) {
    check_table(alphas, total);
    check_ksampler(k, alphas, total);
    if (n_steps == 0 || n_steps > (size_t)total) bad("ksampler: n_steps out of range");
    if (ts_out) ts_out->clear();
    const double smin = k.sigma_min != 0.0 ? k.sigma_min : Table::sigma((double)alphas[0]);
    const double smax = k.sigma_max != 0.0 ? k.sigma_max : Table::sigma((double)alphas[total - 1]);
    const size_t n = n_steps;
    std::vector<double> sg;
    auto frac = [&](size_t i) { return (double)i / (double)(n - 1); };   // (n >= 2 where it is called)
    if (k.schedule == 0) {
        const size_t step = (size_t)total / n;   // sample_latent's schedule (stablediffusion/mod.rs:111,123), quirk Q5 included
        for (long long t = (long long)total - 1; t >= 0; t -= (long long)step) {
            sg.push_back(Table::sigma((double)alphas[t]));
            if (ts_out) ts_out->push_back((int)t);
        }
    } else if (k.schedule == 1) {
        const double rho = k.rho != 0.0 ? k.rho : 7.0;
        const double a = std::pow(smax, 1.0 / rho), b = std::pow(smin, 1.0 / rho);
        for (size_t i = 0; i < n; ++i) sg.push_back(i == 0 ? smax : i == n - 1 ? smin : std::pow(a + frac(i) * (b - a), rho));
    } else if (k.schedule == 2) {
        const double a = std::log(smax), b = std::log(smin);
        for (size_t i = 0; i < n; ++i) sg.push_back(i == 0 ? smax : i == n - 1 ? smin : std::exp(a + frac(i) * (b - a)));
    } else {
        const Table tb(alphas, total);
        for (size_t i = 0; i < n; ++i) {
            const double t = i == 0 ? (double)(total - 1) : i == n - 1 ? 0.0 : (double)(total - 1) * (1.0 - frac(i));
            const int lo = std::min((int)std::floor(t), std::max(total - 2, 0)), hi = std::min(lo + 1, total - 1);
            const double w = t - (double)lo;
            // (at a table entry the entry itself, not exp(ln S_j): the schedule starts at S_total-1 and ends at S_0 exactly)
            sg.push_back(w == 0.0 ? Table::sigma((double)alphas[lo]) : w == 1.0 ? Table::sigma((double)alphas[hi])
                                                                                  : std::exp((1.0 - w) * tb.ln_s[(size_t)lo] + w * tb.ln_s[(size_t)hi]));
        }
    }
    sg.push_back(0.0);
    return sg;
}

std::vector<double> ksampler_plan(const sdmi_ksampler& k, const float* alphas, int total, size_t n_steps, double strength, int* call_steps, int prediction) {
    if (prediction != 0 && prediction != 1) bad("ksampler_plan: prediction must be 0 (eps) or 1 (v)");
    std::vector<int> ts;
    const std::vector<double> sg = ksampler_sigmas(k, alphas, total, n_steps, &ts);
    if (!(strength > 0.0 && strength <= 1.0)) bad("ksampler_plan: strength must satisfy 0 < strength <= 1");
    const size_t L = sg.size() - 1, run = std::min(L, (size_t)(strength * (double)L));   // the img2img rule on steps (sdmi_img2img_timesteps)
    if (run < 1) bad("ksampler_plan: strength * steps leaves no step");
    if (call_steps) *call_steps = (int)run;
    const Table tb(alphas, total);
    auto node = [&](size_t i) { return k.schedule == 0 && i < L ? node_of_table(alphas, ts[i]) : node_of(tb, sg[i]); };
    std::vector<double> rows;
    auto push = [&](size_t step, int stage, const Node& at, Row r, double a_end) {
        if (prediction == 1) {   // eps = a v + b x at the evaluation (ksampler.hpp)
            const double a = 1.0 / std::sqrt(1.0 + at.s * at.s), b = at.s / std::sqrt(1.0 + at.s * at.s);
            r.cx += r.ce * b; r.ce *= a; r.qx += r.qe * b; r.qe *= a;
        }
        const double v[KPLAN_COLS] = {(double)step, (double)stage, at.t, at.s, r.cx, r.ce, r.h1, r.cz, r.cz2, r.qx, r.qe, a_end};
        rows.insert(rows.end(), v, v + KPLAN_COLS);
    };
    const double eta = k.eta;
    for (size_t i = L - run; i < L; ++i) {
        const Node c = node(i), p = node(i + 1);
        const bool first = i == L - run;
        const Node last = first ? c : node(i - 1);
        const double s = c.s, s2 = p.s;
        if (k.kind == 1 || (k.kind == 6 && (s2 <= 0.0))) { push(i, 0, c, dpmpp_2m_row(c, p, first ? nullptr : &last), p.a); continue; }
        if (k.kind == 0 || s2 <= 0.0) { push(i, 0, c, euler_row(c, p, eta), p.a); continue; }   // s' = 0: x_k' = D for every kind
        if (k.kind == 6) {
            const double h = lambda(p) - lambda(c), g = eta * h, B = -std::expm1(-h - g);
            double w0 = 1.0, w1 = 0.0;
            if (!first) {
                const double rr = (lambda(c) - lambda(last)) / h;
                w0 = 1.0 + 1.0 / (2.0 * rr);
                w1 = -1.0 / (2.0 * rr);
            }
            Row r = vp_row(c, p, s2 / s * std::exp(-g) + B * w0, -s * B * w0, B * w1, s2 * std::sqrt(-std::expm1(-2.0 * g)), 0.0);
            r.qx = 1.0 / std::sqrt(c.a); r.qe = -s;   // q = D
            push(i, 0, c, r, p.a);
            continue;
        }
        if (k.kind == 2) {          // heun: Euler to s', then the trapezoid with e2 taken there
            Row r1 = vp_row(c, p, 1.0, s2 - s, 0.0, 0.0, 0.0);
            r1.qe = 1.0;            // q = e1
            push(i, 0, c, r1, -1.0);
            push(i, 1, p, vp_row(p, p, 1.0, 0.5 * (s2 - s), -0.5 * (s2 - s), 0.0, 0.0), p.a);
            continue;
        }
        if (k.kind == 3) {          // dpm2: Euler to the log-midpoint, then the full step with e2 taken there
            const Node m = node_of(tb, std::sqrt(s * s2));
            Row r1 = vp_row(c, m, 1.0, m.s - s, 0.0, 0.0, 0.0);
            r1.qe = 1.0;
            push(i, 0, c, r1, -1.0);
            push(i, 1, m, vp_row(m, p, 1.0, s2 - s, -(m.s - s), 0.0, 0.0), p.a);   // x_k = x2 - e1 (s_m - s)
            continue;
        }
        if (k.kind == 4) {          // dpmpp_2s
            double d, u;
            anc(s, s2, eta, &d, &u);
            const Node m = node_of(tb, std::sqrt(s * d));
            Row r1 = vp_row(c, m, 1.0, m.s - s, 0.0, 0.0, 0.0);   // (s_m / s) x_k + (1 - s_m / s) (x_k - s e)
            r1.qx = 1.0 / std::sqrt(c.a);                         // q = the step's start latent
            push(i, 0, c, r1, -1.0);
            push(i, 1, m, vp_row(m, p, 1.0 - d / s, -(1.0 - d / s) * m.s, d / s, u, 0.0), p.a);
            continue;
        }
        {                           // dpmpp_sde at r = 1/2
            const Node m = node_of(tb, std::sqrt(s * s2));
            double d1, u1, d2, u2;
            anc(s, m.s, eta, &d1, &u1);
            anc(s, s2, eta, &d2, &u2);
            Row r1 = vp_row(c, m, 1.0, d1 - s, 0.0, u1, 0.0);     // (d1 / s) x_k + (1 - d1 / s) (x_k - s e) + u1 z_a
            r1.qx = 1.0 / std::sqrt(c.a);
            push(i, 0, c, r1, -1.0);
            const double al = std::sqrt((s - m.s) / (s - s2)), be = std::sqrt((m.s - s2) / (s - s2));
            push(i, 1, m, vp_row(m, p, 1.0 - d2 / s, -(1.0 - d2 / s) * m.s, d2 / s, u2 * al, u2 * be), p.a);
        }
    }
    return rows;
}

}  // namespace sdmi
