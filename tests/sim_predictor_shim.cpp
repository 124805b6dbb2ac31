// Host build of csrc/fleet_predict.hpp for tests/test_sim_predictor_host.py: the header compiled alone with the host compiler
// (g++ -ffp-contract=off), against sim.PredictorModel. With -DSIM_PREDICTOR_SHIM_MAIN the file is a stand-alone program that runs seeded
// random objects on small tables, duplicated rows and both ends included (built with -fsanitize=address,undefined by the test, run once,
// exit status 0).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../graphbasedlocaltrajectoryplanner_amd/csrc/fleet_predict.hpp"

extern "C" {

// one evaluation of one planner. params[4] = mode, horizon, relax, d_max; table columns s, x, y of n rows; objs: [cnt][5] = x, y, px, py, v;
// points: [cnt][K][2]; outcome: [cnt]; rec: [11], the counters of this evaluation (d_abs_max: the largest here)
void predictor_eval_host(const double* params, const double* s, const double* x, const double* y, int n, int K, const double* objs, int cnt,
                         double* points, int* outcome, double* rec)
{
    const fleet::PredParams P{params[0], params[1], params[2], params[3]};
    const fleet::PredTable R{s, x, y, n};
    for (int c = 0; c < fleet::PRS_DOUBLES; ++c) rec[c] = 0.0;
    rec[fleet::PRS_TICKS] = 1.0; rec[fleet::PRS_N_OBJ] = (double)cnt;
    for (int i = 0; i < cnt; ++i) {
        const double* o = objs + (size_t)5 * i;
        const int istar = P.mode == 2.0 && o[4] > 0.0 ? fleet::pred_nearest(R, o[0], o[1]) : 0;
        const fleet::PredProj pr = fleet::pred_project(P, R, istar, o[0], o[1], o[2], o[3], o[4]);
        outcome[i] = pr.outcome;
        rec[fleet::PRS_OUTCOME0 + pr.outcome] += 1.0;
        if (pr.outcome == fleet::kPredTrack && fleet::pred_abs(pr.d) > rec[fleet::PRS_D_MAX]) rec[fleet::PRS_D_MAX] = fleet::pred_abs(pr.d);
        for (int j = 1; j <= K; ++j) {
            const fleet::PredPoint pt = fleet::pred_point(P, R, K, j, pr, o[0], o[1], o[2], o[3], o[4]);
            points[((size_t)i * K + (j - 1)) * 2] = pt.x; points[((size_t)i * K + (j - 1)) * 2 + 1] = pt.y;
            if (pt.wrapped) rec[fleet::PRS_N_WRAP] += 1.0;
        }
    }
}

}

#ifdef SIM_PREDICTOR_SHIM_MAIN
namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uni()      // xorshift64*: [0, 1)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
}

int main()
{
    long objects = 0, track = 0, wraps = 0;
    for (int n : {2, 3, 7, 64, 65, 200}) {
        // a closed loop of n rows around the origin, radius 50; every third table carries a duplicated row
        std::vector<double> s((size_t)n), x((size_t)n), y((size_t)n);
        for (int i = 0; i < n; ++i) {
            const double a = 6.283185307179586 * (double)i / (double)n;
            x[(size_t)i] = 50.0 * std::cos(a); y[(size_t)i] = 50.0 * std::sin(a);
        }
        if (n % 3 == 0) { x[(size_t)n / 2] = x[(size_t)n / 2 - 1]; y[(size_t)n / 2] = y[(size_t)n / 2 - 1]; }
        s[0] = 1.5;
        for (int i = 1; i < n; ++i) s[(size_t)i] = s[(size_t)i - 1] + std::sqrt((x[(size_t)i] - x[(size_t)i - 1]) * (x[(size_t)i] - x[(size_t)i - 1]) + (y[(size_t)i] - y[(size_t)i - 1]) * (y[(size_t)i] - y[(size_t)i - 1]));
        for (int K = 1; K <= fleet::kPredMaxPoints; ++K)
            for (int mode = 0; mode < 3; ++mode) {
                const int cnt = (int)(uni() * 97.0) % 97;
                std::vector<double> objs((size_t)(cnt > 0 ? cnt : 1) * 5), pts((size_t)(cnt > 0 ? cnt : 1) * K * 2);
                std::vector<int> oc((size_t)(cnt > 0 ? cnt : 1));
                for (int i = 0; i < cnt; ++i) {
                    double* o = &objs[(size_t)5 * i];
                    o[0] = 120.0 * uni() - 60.0; o[1] = 120.0 * uni() - 60.0; o[2] = o[0] + 4.0 * uni() - 2.0; o[3] = o[1] + 4.0 * uni() - 2.0;
                    o[4] = i % 7 == 0 ? 0.0 : 400.0 * uni();
                }
                const double params[4] = {(double)mode, 0.2 + 4.0 * uni(), uni(), K % 2 ? 5.0 : INFINITY};
                double rec[fleet::PRS_DOUBLES];
                predictor_eval_host(params, s.data(), x.data(), y.data(), n, K, objs.data(), cnt, pts.data(), oc.data(), rec);
                double sum = 0.0;
                for (int c = 0; c < fleet::kPredOutcomes; ++c) sum += rec[fleet::PRS_OUTCOME0 + c];
                if (sum != (double)cnt || rec[fleet::PRS_N_WRAP] > (double)cnt * K) { std::fprintf(stderr, "predictor shim: record\n"); return 1; }
                objects += cnt; track += (long)rec[fleet::PRS_OUTCOME0 + fleet::kPredTrack]; wraps += (long)rec[fleet::PRS_N_WRAP];
            }
    }
    std::printf("predictor shim: %ld objects, %ld along the track, %ld wraps\n", objects, track, wraps);
    return 0;
}
#endif
