/*
 * ref_driver -- runs the reference planner class on one described case and dumps what
 * its public surface shows.  TEST INFRASTRUCTURE ONLY: it is built into oracle/_ref/
 * from the reference's own, unmodified sources (oracle/Makefile, target `ref`), and is
 * what tests/golden/gen_golden_ref.py records the ref_* fixtures with.
 *
 *   ref_driver DIR
 *
 * DIR/case.txt holds `key v0 v1 ...` lines (family is a word, the rest numbers);
 * DIR/in_NAME.bin are raw little-endian arrays (float64, or uint8 for `image`).  The
 * driver writes DIR/out_NAME.bin and DIR/manifest.txt (`NAME dtype n0 [n1]` per line).
 * Only public members are used: the methods, getGlobalNode(i, j), the public vectors.
 *
 * Families (tests/ref_ffi.py documents the keys): setcost, costmap, early, path, local.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "DyMu.hpp"

using namespace PathPlanning_lib;
typedef std::vector<std::vector<double>> Matrix;

static std::string g_dir;
static std::map<std::string, std::vector<double>> g_case;
static std::string g_family;
static std::ofstream g_manifest;

static void die(const std::string& msg)
{
    fprintf(stderr, "ref_driver: %s\n", msg.c_str());
    exit(2);
}

static void readCase()
{
    std::ifstream f(g_dir + "/case.txt");
    if (!f) die("no case.txt");
    std::string line;
    while (std::getline(f, line))
    {
        std::istringstream s(line);
        std::string key;
        if (!(s >> key)) continue;
        if (key == "family")
        {
            s >> g_family;
            continue;
        }
        std::vector<double> v;
        std::string tok;
        while (s >> tok) v.push_back(strtod(tok.c_str(), NULL));  // hex floats round-trip
        g_case[key] = v;
    }
}

static const std::vector<double>& vals(const std::string& key)
{
    if (!g_case.count(key)) die("missing key " + key);
    return g_case[key];
}
static double num(const std::string& key, int k = 0) { return vals(key).at(k); }
static bool has(const std::string& key) { return g_case.count(key) != 0; }

template <class T> static std::vector<T> readRaw(const std::string& name)
{
    std::ifstream f(g_dir + "/in_" + name + ".bin", std::ios::binary);
    if (!f) die("missing input " + name);
    f.seekg(0, std::ios::end);
    size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<T> v(bytes / sizeof(T));
    f.read((char*)v.data(), bytes);
    return v;
}

static Matrix readMatrix(const std::string& name, uint nx, uint ny)
{
    std::vector<double> v = readRaw<double>(name);
    if (v.size() != (size_t)nx * ny) die("bad size of " + name);
    Matrix m(ny, std::vector<double>(nx));
    for (uint j = 0; j < ny; j++)
        for (uint i = 0; i < nx; i++) m[j][i] = v[(size_t)j * nx + i];
    return m;
}

template <class T>
static void writeRaw(const std::string& name, const char* dtype, const std::vector<T>& v, long n0,
                     long n1 = -1)
{
    std::ofstream f(g_dir + "/out_" + name + ".bin", std::ios::binary);
    f.write((const char*)v.data(), v.size() * sizeof(T));
    g_manifest << name << " " << dtype << " " << n0;
    if (n1 >= 0) g_manifest << " " << n1;
    g_manifest << "\n";
}
static void writeF64(const std::string& name, const std::vector<double>& v, long n0, long n1 = -1)
{
    writeRaw(name, "f64", v, n0, n1);
}
static void writeI64(const std::string& name, const std::vector<int64_t>& v, long n0, long n1 = -1)
{
    writeRaw(name, "i64", v, n0, n1);
}
static void writeMatrix(const std::string& name, const Matrix& m)
{
    std::vector<double> v;
    for (size_t j = 0; j < m.size(); j++) v.insert(v.end(), m[j].begin(), m[j].end());
    writeF64(name, v, m.size(), m.empty() ? 0 : m[0].size());
}
static void writeScalar(const std::string& name, int64_t x)
{
    writeI64(name, std::vector<int64_t>(1, x), 1);
}

static base::Waypoint wp(double x, double y, double heading = 0.0)
{
    base::Waypoint w;
    w.position[0] = x;
    w.position[1] = y;
    w.heading = heading;
    return w;
}

static void writePathList(const std::string& name, const std::vector<base::Waypoint>& p)
{
    std::vector<double> v;
    for (size_t k = 0; k < p.size(); k++)
    {
        v.push_back(p[k].position[0]);
        v.push_back(p[k].position[1]);
        v.push_back(p[k].position[2]);
        v.push_back(p[k].heading);
    }
    writeF64(name, v, p.size(), 4);
}

struct Grid
{
    uint nx, ny;
    double gres, lres;
    std::vector<double> offset;
};

static Grid readGrid()
{
    Grid g;
    g.nx = (uint)num("nx");
    g.ny = (uint)num("ny");
    g.gres = num("gres");
    g.lres = num("lres");
    g.offset = vals("offset");
    return g;
}

static DyMuPathPlanner* newPlanner(const Grid& g)
{
    int approach = has("approach") ? (int)num("approach") : 0;
    DyMuPathPlanner* p = new DyMuPathPlanner(num("risk_distance"),
                                             num("reconnect_distance"),
                                             num("risk_ratio"),
                                             approach ? SWEEPING : CONSERVATIVE);
    if (!p->initGlobalLayer(g.gres, g.lres, g.nx, g.ny, g.offset)) die("initGlobalLayer");
    return p;
}

// per-node fields through getGlobalNode
static void writeNodeFields(DyMuPathPlanner* p, const Grid& g, const std::string& sfx,
                            const std::vector<std::string>& modes, bool costFields)
{
    size_t n = (size_t)g.nx * g.ny;
    std::vector<double> slope(n), raw(n), cost(n), hazard(n), traff(n);
    std::vector<int64_t> terrain(n), obst(n), loc(n);
    for (uint j = 0; j < g.ny; j++)
        for (uint i = 0; i < g.nx; i++)
        {
            globalNode* q = p->getGlobalNode(i, j);
            size_t k = (size_t)j * g.nx + i;
            obst[k] = q->isObstacle ? 1 : 0;
            cost[k] = q->cost;
            hazard[k] = q->hazard_density;
            traff[k] = q->trafficability;
            if (!costFields) continue;
            slope[k] = q->slope;
            raw[k] = q->raw_cost;
            terrain[k] = q->terrain;
            loc[k] = -1;
            for (size_t m = 0; m < modes.size(); m++)
                if (q->nodeLocMode == modes[m]) loc[k] = (int64_t)m;
            if (loc[k] < 0 && q->nodeLocMode != "DONT_CARE") loc[k] = -2;
        }
    writeI64("is_obstacle" + sfx, obst, g.ny, g.nx);
    writeF64("cost" + sfx, cost, g.ny, g.nx);
    writeF64("hazard" + sfx, hazard, g.ny, g.nx);
    writeF64("traff" + sfx, traff, g.ny, g.nx);
    if (!costFields) return;
    writeF64("slope" + sfx, slope, g.ny, g.nx);
    writeF64("raw_cost" + sfx, raw, g.ny, g.nx);
    writeI64("terrain" + sfx, terrain, g.ny, g.nx);
    writeI64("loc_mode" + sfx, loc, g.ny, g.nx);
}

static std::vector<std::string> modeNames()
{
    std::vector<std::string> m;
    int n = (int)num("n_locs");
    for (int k = 0; k < n; k++) m.push_back("mode" + std::to_string(k));
    return m;
}

static bool runCostMap(DyMuPathPlanner* p, const Grid& g, const std::vector<std::string>& modes)
{
    return p->computeCostMap(readRaw<double>("lut"),
                             readRaw<double>("slopes"),
                             modes,
                             readMatrix("elevation", g.nx, g.ny),
                             readMatrix("terrain", g.nx, g.ny));
}

static void writeNodeList(const std::string& name, const std::vector<globalNode*>& l)
{
    std::vector<int64_t> v;
    for (size_t k = 0; k < l.size(); k++)
    {
        v.push_back((int64_t)l[k]->pose.position[0]);
        v.push_back((int64_t)l[k]->pose.position[1]);
    }
    writeI64(name, v, l.size(), 2);
}

/* ---------------------------------------------------------------- setcost */
static void familySetCost()
{
    Grid g = readGrid();
    DyMuPathPlanner* p = newPlanner(g);
    Matrix wrong(g.ny + 1, std::vector<double>(g.nx, 1.0));
    writeScalar("rc_setcost_wrong_shape", p->setCostMap(wrong));
    writeScalar("rc_setcost", p->setCostMap(readMatrix("cost", g.nx, g.ny)));
    writeScalar("rc_solve_no_goal", p->computeEntireTotalCostMap());
    std::vector<double> probes = readRaw<double>("goal_probes");  // rows of (x, y)
    std::vector<int64_t> rc;
    for (size_t k = 0; k + 1 < probes.size(); k += 2)
    {
        // a fresh planner per probe: an accepted probe must not become the goal
        DyMuPathPlanner* q = newPlanner(g);
        q->setCostMap(readMatrix("cost", g.nx, g.ny));
        bool ok = q->setGoal(wp(probes[k], probes[k + 1]));
        rc.push_back(ok);
        rc.push_back(ok ? (int64_t)q->global_goal->pose.position[0] : -1);
        rc.push_back(ok ? (int64_t)q->global_goal->pose.position[1] : -1);
    }
    writeI64("rc_goal_probes", rc, rc.size() / 3, 3);
    bool ok = p->setGoal(wp(num("goal", 0), num("goal", 1), num("goal", 2)));
    writeScalar("rc_setgoal", ok);
    std::vector<int64_t> node(2, -1);
    if (ok)
    {
        node[0] = (int64_t)p->global_goal->pose.position[0];
        node[1] = (int64_t)p->global_goal->pose.position[1];
    }
    writeI64("goal_node", node, 2);
    writeScalar("rc_solve", p->computeEntireTotalCostMap());
    writeMatrix("total_cost", p->getTotalCostMatrix());
    writeMatrix("global_cost", p->getGlobalCostMatrix());
    writeMatrix("hazard_matrix", p->getHazardDensityMatrix());
    writeMatrix("traff_matrix", p->getTrafficabilityMatrix());
    writeNodeFields(p, g, "", std::vector<std::string>(), false);
}

/* ---------------------------------------------------------------- costmap */
static void familyCostMap()
{
    Grid g = readGrid();
    DyMuPathPlanner* p = newPlanner(g);
    std::vector<std::string> modes = modeNames();
    writeScalar("rc_1", runCostMap(p, g, modes));
    writeNodeFields(p, g, "_1", modes, true);
    writeScalar("rc_2", runCostMap(p, g, modes));
    writeNodeFields(p, g, "_2", modes, true);
}

/* ---------------------------------------------------------------- early */
static void earlyPhase(DyMuPathPlanner* p, const Grid& g, const std::string& sfx,
                       const std::vector<double>& goal, const std::vector<double>& start)
{
    writeScalar("rc_setgoal" + sfx, p->setGoal(wp(goal[0], goal[1])));
    writeScalar("rc" + sfx, p->computeTotalCostMap(wp(start[0], start[1])));
    writeMatrix("total_cost" + sfx, p->getTotalCostMatrix());
    std::vector<int64_t> state((size_t)g.nx * g.ny);
    for (uint j = 0; j < g.ny; j++)
        for (uint i = 0; i < g.nx; i++)
            state[(size_t)j * g.nx + i] = p->getGlobalNode(i, j)->state == CLOSED ? 1 : 0;
    writeI64("closed" + sfx, state, g.ny, g.nx);
    writeNodeList("narrowband" + sfx, p->global_narrowband);
    writeNodeList("propagated" + sfx, p->global_propagated_nodes);
    std::vector<int64_t> next(2, -1);
    if (!p->global_narrowband.empty())
    {
        globalNode* q = p->minCostGlobalNode();  // also erases it from the band
        next[0] = (int64_t)q->pose.position[0];
        next[1] = (int64_t)q->pose.position[1];
    }
    writeI64("next_min" + sfx, next, 2);
}

static void familyEarly()
{
    Grid g = readGrid();
    DyMuPathPlanner* p = newPlanner(g);
    p->setCostMap(readMatrix("cost", g.nx, g.ny));
    earlyPhase(p, g, "_1", vals("goal"), vals("start"));
    p->resetTotalCostMap();
    writeMatrix("total_cost_reset", p->getTotalCostMatrix());
    writeScalar("propagated_after_reset", (int64_t)p->global_propagated_nodes.size());
    earlyPhase(p, g, "_2", vals("goal2"), vals("start2"));
}

/* ---------------------------------------------------------------- path */
static void familyPath()
{
    Grid g = readGrid();
    DyMuPathPlanner* p = newPlanner(g);
    std::vector<std::string> modes = modeNames();
    runCostMap(p, g, modes);
    writeScalar("rc_setgoal", p->setGoal(wp(num("goal", 0), num("goal", 1), num("goal", 2))));
    writeScalar("rc_solve", p->computeEntireTotalCostMap());
    writeMatrix("total_cost", p->getTotalCostMatrix());
    writeNodeFields(p, g, "", modes, true);
    std::vector<double> starts = readRaw<double>("starts");  // rows of (x, y, heading)
    std::vector<int64_t> len;
    std::vector<base::Waypoint> all;
    for (size_t k = 0; k + 2 < starts.size(); k += 3)
    {
        std::vector<base::Waypoint> path = p->getPath(wp(starts[k], starts[k + 1], starts[k + 2]));
        len.push_back((int64_t)path.size());
        all.insert(all.end(), path.begin(), path.end());
    }
    writeI64("path_len", len, len.size());
    writePathList("path_wp", all);
    std::vector<double> pts = readRaw<double>("points");  // rows of (x, y)
    std::vector<double> tc;
    std::vector<int64_t> loc;
    for (size_t k = 0; k + 1 < pts.size(); k += 2)
    {
        tc.push_back(p->getTotalCost(wp(pts[k], pts[k + 1])));
        std::string m = p->getLocomotionMode(wp(pts[k], pts[k + 1]));
        int64_t idx = m == "DONT_CARE" ? -1 : -2;
        for (size_t q = 0; q < modes.size(); q++)
            if (m == modes[q]) idx = (int64_t)q;
        loc.push_back(idx);
    }
    writeF64("point_cost", tc, tc.size());
    writeI64("point_loc", loc, loc.size());
}

/* ---------------------------------------------------------------- local */
static void familyLocal()
{
    Grid g = readGrid();
    DyMuPathPlanner* p = newPlanner(g);
    std::vector<std::string> modes = modeNames();
    runCostMap(p, g, modes);
    writeScalar("rc_setgoal", p->setGoal(wp(num("goal", 0), num("goal", 1), num("goal", 2))));
    writeScalar("rc_solve", p->computeEntireTotalCostMap());
    writeMatrix("total_cost", p->getTotalCostMatrix());
    writePathList("path", p->getPath(wp(num("start", 0), num("start", 1), num("start", 2))));
    if (!has("rover"))  // first stage only: the caller builds the image from this path
        return;
    base::samples::frame::Frame frame;
    frame.image = readRaw<uint8_t>("image");
    frame.width = (uint16_t)num("image_size", 0);
    frame.height = (uint16_t)num("image_size", 1);
    frame.pixel_size = (uint32_t)num("image_size", 2);
    frame.row_size = frame.width * frame.pixel_size;
    if (frame.image.size() != (size_t)frame.row_size * frame.height) die("bad image size");
    base::Waypoint rover = wp(num("rover", 0), num("rover", 1));
    std::vector<base::Waypoint> trajectory;
    base::Time t;
    writeScalar("rc_local", p->computeLocalPlanning(rover, frame, num("image_res"), trajectory, t));
    writePathList("trajectory", trajectory);
    writePathList("current_path", p->current_path);
    writeScalar("reconnecting_index", p->getReconnectingIndex());
    writeMatrix("risk", p->getRiskMatrix(rover));
    writeMatrix("deviation", p->getDeviationMatrix(rover));
    writeMatrix("hazard_matrix", p->getHazardDensityMatrix());
    writeMatrix("traff_matrix", p->getTrafficabilityMatrix());
    writeMatrix("global_cost", p->getGlobalCostMatrix());
    writeScalar("rc_resolve", p->computeEntireTotalCostMap());
    writeMatrix("total_cost_2", p->getTotalCostMatrix());
}

int main(int argc, char** argv)
{
    if (argc != 2) die("usage: ref_driver DIR");
    g_dir = argv[1];
    readCase();
    g_manifest.open(g_dir + "/manifest.txt");
    if (g_family == "setcost")
        familySetCost();
    else if (g_family == "costmap")
        familyCostMap();
    else if (g_family == "early")
        familyEarly();
    else if (g_family == "path")
        familyPath();
    else if (g_family == "local")
        familyLocal();
    else
        die("unknown family '" + g_family + "'");
    g_manifest.close();
    return 0;
}
