// Host build of csrc/fleet_select.hpp for tests/test_sim_selector_host.py: the header compiled alone with the host compiler
// (g++ -ffp-contract=off), against sim.SelectorModel.
#include <cstdint>

#include "../graphbasedlocaltrajectoryplanner_amd/csrc/fleet_select.hpp"

extern "C" {

// one evaluation. params[6] = horizon, r_ego, c_hard, c_soft, w_clear, w_switch; user[L]; n_rows[5]: per action straight .. right and
// emergency -1 (not exported) or the rows; rows: [4][4][256] = per action the columns s, x, y, vx; objs: [cnt][5] = x, y, px, py, r.
// Out: order[L], act_d[4][3] = vbar, clear, J, act_i[4][2] = clear_obj, flags; rec[12]: updated in place
void selector_eval_host(const double* params, const int* user, int L, int sel_prev, const int* n_rows, const double* rows, const double* objs, int cnt,
                        int* order, double* act_d, int* act_i, double* rec)
{
    const fleet::SelParams P{params[0], params[1], params[2], params[3], params[4], params[5]};
    fleet::SelAct act[fleet::kSelActions];
    fleet::sel_case(P, user, L, sel_prev, n_rows, rows, objs, cnt, order, act, rec);
    for (int a = 0; a < fleet::kSelActions; ++a) {
        act_d[3 * a] = act[a].vbar; act_d[3 * a + 1] = act[a].clear; act_d[3 * a + 2] = act[a].J;
        act_i[2 * a] = act[a].clear_obj; act_i[2 * a + 1] = act[a].flags;
    }
}

int selector_record_doubles() { return fleet::SLS_DOUBLES; }

}
