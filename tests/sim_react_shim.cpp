// Host build of csrc/fleet_react.hpp for tests/test_sim_react_host.py: the header compiled alone with the host compiler
// (g++ -ffp-contract=off), against sim.ReactModel / sim.react_tick.
#include "../graphbasedlocaltrajectoryplanner_amd/csrc/fleet_react.hpp"

extern "C" {

int react_record_doubles() { return fleet::RCT_DOUBLES; }
int react_param_doubles() { return (int)(sizeof(fleet::ReactParams) / sizeof(double)); }

// the start state of a record [16]
void react_start_host(double* rec) { fleet::react_start(rec); }

// one tick: params[9] = on, a_max, b_comf, b_max, headway, gap0, look, lat_gate, ego_len; the race table's columns S, X, Y, V of n_rl rows;
// the ego's x, y, v; opp[n][4] = s, c, e, length; rec[16] in and out; e_out[n]; per_opp[n][4] = leader, delta, gap, acc; ego_out[3] = s_e,
// d_e, has
void react_tick_host(const double* params, const double* S, const double* X, const double* Y, const double* V, int n_rl, double x, double y,
                     double v, double dt, double tick, const double* opp, int n, double* rec, double* e_out, double* per_opp, double* ego_out)
{
    const fleet::ReactParams P{params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7], params[8]};
    fleet::react_tick_host(P, fleet::ReactTable{S, X, Y, V, n_rl}, x, y, v, dt, tick, opp, n, rec, e_out, per_opp, ego_out);
}

}
