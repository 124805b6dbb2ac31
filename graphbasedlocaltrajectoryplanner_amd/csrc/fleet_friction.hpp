// fleet_friction.hpp -- included at the end of ltpl_hip.hip. FRICTION MAPS of a fleet (include/ltpl_hip.h, additive to ABI v9): location
// dependent grip (local_gg as a dict, OTH.py:633-666) from grids that live in device memory, so that the rows of a tick are evaluated
// where the stitched paths already lie -- inside stage A of the velocity stage (fleet_core.hpp vel_a<X, true>, fleet::friction_at) -- and
// the closed-loop simulation, a tape and the per-call fleet all drive on a map without a host round trip per tick.
//
//   ltpl_fleet_friction        maps + map / grip factor of every planner (n_maps = 0 clears)
//   ltpl_fleet_friction_scale  grip factors only
//   ltpl_fleet_friction_rows   k_friction_rows: batched lookup, one lane per point (the test hook of the interpolation)

__global__ __launch_bounds__(256) void k_friction_rows(fleet::FrMap m, const double* nodes, const double* x, const double* y, int n, double scale, double* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const fleet::FrVal a = fleet::friction_at(m, nodes, x[i], y[i], scale);
    *reinterpret_cast<fleet::FrVal*>(out + (size_t)i * 2) = a;
}

// every argument is checked before the first HIP call
static int friction_check(ltpl_fleet* f, const ltpl_fleet_friction_in* in, std::vector<fleet::FrMap>* maps, bool* on)
{
    const int N = f->D.N;
    auto bad = [&](const char* why, int code = LTPL_ERR_INVALID_ARG) { f->err = std::string("fleet friction: ") + why; return code; };
    if (in->n_maps < 0) return bad("n_maps must not be negative");
    *on = false;
    if (in->n_maps == 0) return LTPL_OK;
    if (!in->x0 || !in->y0 || !in->dx || !in->dy || !in->nx || !in->ny || !in->node_off || !in->nodes) return bad("map arrays missing");
    if (!in->map_idx || !in->scale) return bad("map_idx / scale missing");
    if (in->node_off[0] != 0) return bad("node_off must start at 0");
    for (int m = 0; m < in->n_maps; ++m) {
        if (in->nx[m] < 2 || in->ny[m] < 2) return bad("a map needs at least 2 x 2 nodes");
        if (!std::isfinite(in->x0[m]) || !std::isfinite(in->y0[m])) return bad("x0 / y0 must be finite");
        if (!std::isfinite(in->dx[m]) || !std::isfinite(in->dy[m]) || !(in->dx[m] > 0.0) || !(in->dy[m] > 0.0)) return bad("dx / dy must be finite and positive");
        const long long cnt = (long long)in->nx[m] * (long long)in->ny[m];
        if (cnt > 0x3fffffffll || (long long)in->node_off[m] + cnt > 0x3fffffffll) return bad("more nodes than a 30-bit index can name", LTPL_ERR_CAPACITY);
        if ((long long)in->node_off[m + 1] - (long long)in->node_off[m] != cnt) return bad("node_off[m + 1] - node_off[m] must be nx[m] * ny[m]");
        maps->push_back(fleet::FrMap{in->x0[m], in->y0[m], in->dx[m], in->dy[m], in->nx[m], in->ny[m], in->node_off[m], 0});
    }
    const size_t nn = (size_t)in->node_off[in->n_maps] * 2;
    for (size_t i = 0; i < nn; ++i) if (!std::isfinite(in->nodes[i]) || !(in->nodes[i] > 0.0)) return bad("node values must be finite and positive");
    for (int p = 0; p < N; ++p) {
        if (in->map_idx[p] < -1 || in->map_idx[p] >= in->n_maps) return bad("map_idx out of range");
        if (!std::isfinite(in->scale[p]) || !(in->scale[p] > 0.0)) return bad("a scale must be finite and positive");
        *on = *on || in->map_idx[p] >= 0;
    }
    if (*on && f->vel_lds_gg > 150 * 1024) return bad("velocity profile with friction rows too long for the LDS-resident solver", LTPL_ERR_CAPACITY);
    return LTPL_OK;
}

struct FrictionAllocs {                      // what a call allocated so far: freed unless the call commits
    std::vector<void*> p;
    ~FrictionAllocs() { for (void* q : p) if (q) (void)hipFree(q); }
};
template <class T>
static int friction_upload(ltpl_fleet* f, FrictionAllocs* a, const T* src, size_t n, T** out)
{
    void* d = nullptr;
    FLEET_TRY(f, hipMalloc(&d, (n ? n : 1) * sizeof(T)));
    a->p.push_back(d);
    if (n) FLEET_TRY(f, hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<T*>(d);
    return LTPL_OK;
}

extern "C" int ltpl_fleet_friction(ltpl_fleet* f, const ltpl_fleet_friction_in* in)
try {
    if (!f || !in) return LTPL_ERR_INVALID_ARG;
    std::vector<fleet::FrMap> maps; bool on = false;
    int rc = friction_check(f, in, &maps, &on);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));      // (no kernel of this fleet is in flight that could read the old maps or the rows pointer)
    const int N = f->D.N;
    // everything new is allocated first: the fleet keeps its previous maps (all of them valid) unless every step succeeds
    FrictionAllocs a;
    fleet::FrMap* d_maps = nullptr; double* d_nodes = nullptr; int* d_idx = nullptr; double* d_scale = nullptr;
    unsigned char* d_gg = nullptr;
    if (in->n_maps > 0) {
        if ((rc = friction_upload(f, &a, maps.data(), maps.size(), &d_maps))) return rc;
        if ((rc = friction_upload(f, &a, in->nodes, (size_t)in->node_off[in->n_maps] * 2, &d_nodes))) return rc;
        if ((rc = friction_upload(f, &a, in->map_idx, (size_t)N, &d_idx))) return rc;
        if ((rc = friction_upload(f, &a, in->scale, (size_t)N, &d_scale))) return rc;
        if (on && !f->d_gg) {                              // the planners' friction rows (as the first call that carries rows allocates them)
            void* g = nullptr;
            FLEET_TRY(f, hipMalloc(&g, f->D.gg_stride * (size_t)N));
            a.p.push_back(g); d_gg = static_cast<unsigned char*>(g);
        }
    }
    // commit (nothing below fails)
    for (void* q : {(void*)f->fr_maps, (void*)f->fr_nodes, (void*)f->fr_idx, (void*)f->fr_scale}) if (q) (void)hipFree(q);
    f->fr_maps = d_maps; f->fr_nodes = d_nodes; f->fr_idx = d_idx; f->fr_scale = d_scale;
    if (d_gg) { f->allocs.push_back(d_gg); f->d_gg = d_gg; f->args.gg = d_gg; }
    a.p.clear();
    f->fr_host.swap(maps); f->fr_on = on;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_friction_scale(ltpl_fleet* f, const double* scale)
try {
    if (!f || !scale) return LTPL_ERR_INVALID_ARG;
    if (!f->fr_scale) { f->err = "fleet friction: ltpl_fleet_friction first"; return LTPL_ERR_INVALID_ARG; }
    for (int p = 0; p < f->D.N; ++p)
        if (!std::isfinite(scale[p]) || !(scale[p] > 0.0)) { f->err = "fleet friction: a scale must be finite and positive"; return LTPL_ERR_INVALID_ARG; }
    int rc = fleet_enter(f);
    if (rc) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FLEET_TRY(f, hipMemcpy(f->fr_scale, scale, sizeof(double) * (size_t)f->D.N, hipMemcpyHostToDevice));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_friction_rows(ltpl_fleet* f, int32_t map, const double* x, const double* y, int32_t n_pts, double scale, double* out)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const char* why) { f->err = std::string("fleet friction: ") + why; return LTPL_ERR_INVALID_ARG; };
    if (n_pts < 0) return bad("n_pts must not be negative");
    if (n_pts > 0 && (!x || !y || !out)) return bad("x / y / out missing");
    if (map < 0 || (size_t)map >= f->fr_host.size()) return bad("map out of range");
    if (!std::isfinite(scale)) return bad("scale must be finite");
    if (n_pts == 0) return LTPL_OK;
    int rc = fleet_enter(f);
    if (rc) return rc;
    const size_t n = (size_t)n_pts;
    double* d = nullptr;
    struct Guard { void* a = nullptr; ~Guard() { if (a) (void)hipFree(a); } } g;
    FLEET_TRY(f, hipMalloc(reinterpret_cast<void**>(&d), 32 * n)); g.a = d;          // x | y | out [n][2]
    FLEET_TRY(f, hipMemcpy(d, x, 8 * n, hipMemcpyHostToDevice));
    FLEET_TRY(f, hipMemcpy(d + n, y, 8 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_friction_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, f->h->stream, f->fr_host[(size_t)map], (const double*)f->fr_nodes,
                       (const double*)d, (const double*)(d + n), (int)n_pts, scale, d + 2 * n);
    FLEET_TRY(f, hipGetLastError());
    FLEET_TRY(f, hipMemcpyAsync(out, d + 2 * n, 16 * n, hipMemcpyDeviceToHost, f->h->stream));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))
