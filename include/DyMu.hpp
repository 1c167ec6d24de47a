// DyMu.hpp -- PathPlanning_lib::DyMuPathPlanner, the global-layer surface of
// the reference class (src/DyMu.hpp:397-609) re-implemented over row-major
// SoA arrays, with the total-cost propagation delegated to the MI355X engine
// through the C-ABI in dymu_fim.h.
//
// Same method names, argument meaning and return values as the reference for
// the hot path and its two neighbours (cost-map ingestion, path extraction):
//   initGlobalLayer      src/DyMu_GlobalPathPlanning.cpp:39-104
//   setCostMap           :109-126
//   computeCostMap       :145-181 (+ :186-308, quirks Q1-Q4 of SURVEY s8(a))
//   setGoal              :322-357
//   computeTotalCostMap  :364-408
//   computeEntireTotalCostMap :443-468
//   getPath / computeGlobalPath :589-662 (+ :666-784)
//   getTotalCostMatrix, getGlobalCostMatrix, getHazardDensityMatrix,
//   getTrafficabilityMatrix, getTotalCost, getLocomotionMode  :788-890
//   local layer (src/DyMu_LocalPathRepairing.cpp, csrc/local_layer.cpp):
//   computeLocalPlanning, repairPath, evaluatePath, expandRisk,
//   computeLocalPropagation, getLocalPath, computeLocalWaypointGDM,
//   getRiskMatrix, getDeviationMatrix, getReconnectingIndex, getLocalNode,
//   subdivideGlobalNode, getTotalCost(localNode)
// Differences a caller can see:
//   * nodes are SoA arrays, not heap records: getGlobalNode /
//     getNearestGlobalNode / getLocalNode return snapshots (std::optional for
//     the reference's NULL), node-taking methods take grid indices or a
//     snapshot; CoRa (cost-ratio learning) is not part of this library.
//   * computeTotalCostMap stops like the reference once the start and its nb4
//     are final: CLOSED cells hold their converged values, the
//     narrow band the reference's tentative values (replayed on the host from
//     the CLOSED values), every other cell +inf; ties between equal total
//     costs follow the reference's insertion order, rebuilt from the values
//     (csrc/pop_order.hpp), and so does the band list.
//   * the node-pointer members are accessors returning snapshots:
//     globalNarrowband(), globalPropagatedNodes(), globalGoal(), localAgent(),
//     localNarrowband(), localExpandableObstacles(), localPropagatedNodes(); a
//     node's public `state` is written through setGlobalNodeState.  The per-node
//     steps of the loops the library runs whole are there too, by grid index or
//     snapshot (propagateGlobalNode, maxRiskNode, propagateRisk,
//     propagateLocalNode, minCostLocalNode x2), so a caller can drive the
//     reference's loops itself.  setHorizonCost (src/DyMu.hpp:555) is declared
//     but defined nowhere in the reference (a caller cannot link it there); it
//     is not provided.
//   * a start or goal on the border returns false instead of dereferencing
//     NULL (reference :416-417, :430-431).
#pragma once

#include <cstdint>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "dymu_base.hpp"
#include "dymu_fim.h"

namespace PathPlanning_lib {

enum node_state { OPEN, CLOSED };

enum repairingAproach {
  CONSERVATIVE,  // Hazard Avoidance - FM*
  SWEEPING       // multiBiFM*
};

// Snapshot of a global node (the reference's globalNode, src/DyMu.hpp:69-108,
// without the neighbour pointer lists and the local map).
struct globalNode {
  base::Pose2D pose;        // grid indices (i, j)
  base::Pose2D world_pose;  // i * res, j * res
  double elevation = 0.0, slope = 0.0;
  node_state state = OPEN;
  bool isObstacle = false;
  bool hasLocalMap = false;
  double raw_cost = 0.0, cost = 0.0, hazard_density = 0.0, trafficability = 1.0;
  double total_cost = 0.0;
  unsigned terrain = 0;
  std::string nodeLocMode = "DONT_CARE";
};

// Snapshot of a local-layer sub-cell (the reference's localNode,
// src/DyMu.hpp:42-67, without nb4List).  id names the sub-cell for the
// node-taking methods below.
struct localNode {
  base::Pose2D pose;         // sub-cell indices inside the parent global node
  base::Pose2D world_pose;   // global_pose / global_res
  base::Pose2D parent_pose;  // parent global node (grid indices)
  base::Pose2D global_pose;  // in global units
  double deviation = 0.0, total_cost = 0.0, cost = 0.0, risk = 0.0;
  node_state state = OPEN;
  bool isObstacle = false;
  uint64_t id = 0;
};

struct LocalLayer;  // csrc/local_layer.hpp
struct PathIndex;   // csrc/local_layer.hpp
struct TieGuard;    // csrc/pop_order.hpp

class DyMuPathPlanner {
 public:
  // -- public state kept from the reference (src/DyMu.hpp:444-467) --
  std::vector<base::Waypoint> current_path;  // the last computed path
  std::vector<double> cost_lutable;          // cost LUT (computeCostMap)
  double remaining_total_cost = 0.0;
  int reconnecting_index = 0;

  DyMuPathPlanner(double risk_distance, double reconnect_distance, double risk_ratio,
                  repairingAproach input_approach);
  ~DyMuPathPlanner();
  DyMuPathPlanner(const DyMuPathPlanner&) = delete;
  DyMuPathPlanner& operator=(const DyMuPathPlanner&) = delete;

  bool initGlobalLayer(double globalres, double localres, unsigned num_nodes_X,
                       unsigned num_nodes_Y, std::vector<double> offset);
  bool setCostMap(std::vector<std::vector<double>> cost_map);
  bool computeCostMap(std::vector<double> cost_data, std::vector<double> slope_values,
                      std::vector<std::string> locomotionModes,
                      std::vector<std::vector<double>> elevation,
                      std::vector<std::vector<double>> terrainMap);
  // the same from row-major nx*ny arrays (the flat C-ABI's path: no per-row copies)
  bool computeCostMap(const std::vector<double>& cost_data,
                      const std::vector<double>& slope_values,
                      const std::vector<std::string>& locomotionModes, const double* elevation,
                      const double* terrainMap);

  // the per-node steps of computeCostMap (src/DyMu.hpp:493-497), by grid index
  void calculateSlope(unsigned i, unsigned j);
  void calculateNominalCost(unsigned i, unsigned j, int range, int numLocs);
  void smoothCost(unsigned i, unsigned j);

  bool setGoal(base::Waypoint wGoal);
  bool computeTotalCostMap(base::Waypoint wPos);
  bool computeEntireTotalCostMap();

  std::vector<base::Waypoint> getPath(base::Waypoint wPos);
  bool computeGlobalPath(base::Waypoint wPos);
  base::Waypoint computeNextGlobalWaypoint(base::Waypoint& wPos, double tau);
  double interpolate(double a, double b, double g00, double g01, double g10, double g11);

  std::string getLocomotionMode(base::Waypoint wPos);
  std::vector<std::vector<double>> getTotalCostMatrix();
  std::vector<std::vector<double>> getGlobalCostMatrix();
  std::vector<std::vector<double>> getHazardDensityMatrix();
  std::vector<std::vector<double>> getTrafficabilityMatrix();
  double getTotalCost(base::Waypoint wInt);

  // -- node-level access (src/DyMu.hpp:500-518); std::nullopt = the reference's NULL --
  std::optional<globalNode> getGlobalNode(unsigned i, unsigned j);
  std::optional<globalNode> getNearestGlobalNode(base::Pose2D pos);
  std::optional<globalNode> getNearestGlobalNode(base::Waypoint wPos);
  std::optional<globalNode> globalGoal();  // the reference's public global_goal
  bool isSafeNode(unsigned i, unsigned j);         // :410-422 (border -> false)
  bool isFullyClosedNode(unsigned i, unsigned j);  // :424-436 (border -> false)
  void resetTotalCostMap();                        // :473-485: every node OPEN at +inf
  // the reference's global_narrowband (:445) as the last computeTotalCostMap left
  // it: snapshots of the band nodes in the reference's insertion order (rebuilt from
  // the values, csrc/pop_order.hpp); empty after computeEntireTotalCostMap
  std::vector<globalNode> globalNarrowband();
  // :548-567: the band node with the lowest total cost (first in insertion order
  // on ties), removed from the band list like the reference's erase; the map is
  // not changed.  std::nullopt on an empty band (the reference reads front()).
  std::optional<globalNode> minCostGlobalNode();
  // :487-498: the band holds only the goal (total cost 0)
  void resetGlobalNarrowBand();
  // :500-546: the reference update of node (i, j) from its nb4's current total costs
  // (a NULL neighbour: the other one alone; C from the node's cost, hazard and
  // trafficability); a lower value is taken, and a node whose total cost was +inf
  // joins the band (appended: insertion order, like the reference's vector) and the
  // propagated list.  Host arithmetic on the host copy of the map: for callers that
  // drive the propagation node by node; the solves run on the GPU.
  void propagateGlobalNode(unsigned i, unsigned j);
  void propagateGlobalNode(const globalNode& n);
  // the reference's public globalNode::state written by a caller (its FMM loop sets
  // CLOSED after each minCostGlobalNode); the next solve recomputes every state
  void setGlobalNodeState(unsigned i, unsigned j, node_state s);
  // global_propagated_nodes (:447): every node with a finite total cost in the
  // reference's insertion order, then those added by propagateGlobalNode.  (At 16384^2
  // after a full solve that is ~2.6e8 snapshots: globalPropagatedCount first.)
  std::vector<globalNode> globalPropagatedNodes();
  // the same list as grid indices (j * nx + i), without the snapshots
  std::vector<uint64_t> globalPropagatedIndices();
  uint64_t globalPropagatedCount();
  // every node's state (ny*nx, row-major: 1 CLOSED, 0 OPEN) as the last solve or the
  // caller's setGlobalNodeState left it (the reference's globalNode::state, in bulk)
  void copyNodeStates(uint8_t* out);
  // :731-784 / L:979-1023: the normalised descent direction at a node (the
  // reference's gradientNode(globalNode*) / gradientNode(localNode*))
  void gradientNode(unsigned i, unsigned j, double& dnx, double& dny) const;
  void gradientNode(const globalNode& n, double& dnx, double& dny) const;
  void gradientNode(const localNode& n, double& dnx, double& dny) const;

  // -- local layer (src/DyMu.hpp:539-591) --
  bool computeLocalPlanning(base::Waypoint wPos, base::samples::frame::Frame traversabilityMap,
                            double res, std::vector<base::Waypoint>& trajectory,
                            base::Time& localTime);
  int repairPath(base::Waypoint wInit, unsigned index);
  bool evaluatePath(unsigned starting_index);
  void expandRisk();
  // the set node, or std::nullopt (the reference's NULL; also after the
  // wall-clock limit, 5 s as in src/DyMu_LocalPathRepairing.cpp:685-696)
  std::optional<localNode> computeLocalPropagation(base::Waypoint wInit, base::Waypoint wOvertake);
  std::vector<base::Waypoint> getLocalPath(const localNode& lSetNode, base::Waypoint wInit,
                                           double tau);
  bool computeLocalWaypointGDM(base::Waypoint& wPos, double tau);
  std::optional<localNode> getLocalNode(base::Waypoint wPos);  // subdivides, like :177-189
  std::optional<localNode> getLocalNode(base::Pose2D pos);     // :160-173
  void subdivideGlobalNode(unsigned i, unsigned j);            // :150-156
  void createLocalMap(unsigned i, unsigned j);                 // :97-148 (as subdivide)
  // L:851-869: the step toward the nb4 sub-cell of lowest deviation
  base::Waypoint computeLocalWaypointDijkstra(const localNode& lNode);
  // the per-node steps of expandRisk / computeLocalPropagation (L:525-576, L:700-805):
  // maxRiskNode pops local_expandable_obstacles by the reference's rule (the front,
  // unless it is below 1 and a later entry is higher: then the first such), nullopt
  // when empty; propagateRisk / propagateLocalNode apply the risk / deviation update
  // to a sub-cell and queue it like the reference; minCostLocalNode pops the band
  // node of lowest deviation (SWEEPING, :752-775) or deviation + distance to
  // reachNode (CONSERVATIVE, :777-805), first strict minimum in insertion order
  // the reference's localNode::nb4List[d] (src/DyMu.hpp:52; d: 0 (i,j-1), 1 (i-1,j),
  // 2 (i+1,j), 3 (i,j+1)): nullopt where the reference holds NULL
  std::optional<localNode> localNeighbour(const localNode& n, int d);
  std::optional<localNode> maxRiskNode();
  // the reference's public localNode::state written by a caller (its loop closes each
  // popped node, L:654)
  void setLocalNodeState(const localNode& n, node_state s);
  void propagateRisk(const localNode& n);
  void propagateLocalNode(const localNode& n);
  std::optional<localNode> minCostLocalNode(double Tovertake, double minC);
  std::optional<localNode> minCostLocalNode(const localNode& reachNode);
  // the reference's public local lists (src/DyMu.hpp:448-454) as snapshots, in their
  // order: local_narrowband (insertion order), local_expandable_obstacles (queue
  // order), local_propagated_nodes (insertion order)
  std::vector<localNode> localNarrowband();
  std::vector<localNode> localExpandableObstacles();
  std::vector<localNode> localPropagatedNodes();
  // L:441-471 against current_path
  bool isBlockingObstacle(const localNode& obNode, unsigned& maxIndex, unsigned& minIndex);
  // the reference's local_agent (src/DyMu.hpp:460): the last local propagation's
  // start sub-cell, std::nullopt before one ran
  std::optional<localNode> localAgent();
  double getTotalCost(const localNode& lNode);                 // :473-491
  std::vector<std::vector<double>> getRiskMatrix(base::Waypoint rover_pos);
  std::vector<std::vector<double>> getDeviationMatrix(base::Waypoint rover_pos);
  int getReconnectingIndex();

  // -- extensions (not in the reference) --
  // computeLocalPropagation's wall-clock limit in seconds (the reference's fixed
  // 5.0, :685-696); <= 0 disables it
  void setLocalPropagationTimeout(double seconds) { local_timeout_s_ = seconds; }
  double localPropagationTimeout() const { return local_timeout_s_; }
  // Flat row-major views for FFI callers (ny*nx, index j*nx + i).  The total
  // cost lives on the device; this downloads whatever the host copy lacks.
  const double* totalCostData() const;
  // The whole total cost into out (ny*nx): raw (+inf unreachable) or as
  // getTotalCostMatrix (-1), row ranges on the host threads.
  void copyTotalCost(double* out, bool raw) const;
  unsigned sizeX() const { return nx_; }
  unsigned sizeY() const { return ny_; }
  bool hasGoal() const { return has_goal_; }
  unsigned goalI() const { return goal_i_; }
  unsigned goalJ() const { return goal_j_; }
  const dymu_stats& lastStats() const { return stats_; }
  // How the last computeTotalCostMap / computeEntireTotalCostMap ran: 0 cold
  // solve, 1 windowed re-propagation from the changed speed window, 2 map reused.
  int lastSolveKind() const { return incremental_; }
  // Local-layer feedback on the global layer (the writes of
  // src/DyMu_LocalPathRepairing.cpp:264-274 and :389-394), row-major ny*nx.
  // Only the rows that differ from the current values are re-packed and
  // uploaded before the next solve.
  bool setHazardDensity(const std::vector<double>& hd);
  bool setTrafficability(const std::vector<double>& tr);
  // Windowed forms: w x h values (row-major) for cells [i0, i0+w) x [j0, j0+h).
  bool setHazardDensityWindow(unsigned i0, unsigned j0, unsigned w, unsigned h,
                              const double* hd);
  bool setTrafficabilityWindow(unsigned i0, unsigned j0, unsigned w, unsigned h,
                               const double* tr);
  // setCostMap for the cells [i0, i0+w) x [j0, j0+h) only: w x h costs, row-major, each
  // applied by setCostMap's per-cell rule.  false, and nothing changes: a null pointer or
  // a box not inside the grid (as the windowed setters above).  Only the rows of the box
  // are re-packed at the next solve, so a converged map follows by the windowed
  // re-propagation; with setGlobalRisk on, obstacles the box adds reach R through the
  // incremental update (below), an obstacle it frees through the whole recompute, or, with
  // trackObstacleRemoval on, through the incremental update as well.
  bool setCostMapWindow(unsigned i0, unsigned j0, unsigned w, unsigned h, const double* cost);
  // Narrow-band cells left by the last computeTotalCostMap (0 after a full solve).
  uint64_t lastBandSize() const { return band_cells_.size(); }
  // How the last computeTotalCostMap resolved the reference's order at its exit
  // value: cells of exactly that value, how many of them the
  // reference had not closed yet, whether the exact host replay ran (degenerate
  // ties only), host time of the resolution and band replay.
  struct EarlyExitInfo {
    uint64_t tied = 0, open_at_limit = 0;
    int exact_replay = 0;         // 1: the exit was replayed exactly on the host
    double resolve_ms = 0.0;
    uint64_t replay_updates = 0;  // reference updates the band replay evaluated
    int band_exact = 1;           // every band value is the reference's (always, since round 6)
    // comparisons of engine values rounding could flip (near ties, pop_order.hpp's
    // TieGuard): any sends the exit to the exact host replay
    uint64_t near_ties = 0;
    unsigned replay_threads = 0;  // host threads of the band replay
  };
  const EarlyExitInfo& lastEarlyExitInfo() const { return early_info_; }
  // Engine options (device ordinal etc.); takes effect on the next solve.
  void setEngineOptions(const dymu_opts& o);
  // Install a total-cost map (ny*nx, +inf unreachable) as the state a
  // converged computeEntireTotalCostMap leaves: every finite node CLOSED (the
  // reference's public globalNode::total_cost / state writes).  The next
  // solve starts cold.  No solve runs here.
  bool loadTotalCostMap(const double* T);
  // Batched path extraction: for each start, the path computeGlobalPath would leave in
  // current_path (the offset removed on entry and added on exit, as getPath does).
  // These are GLOBAL paths: getPaths does not run evaluatePath and does not touch
  // current_path.  While the device map holds what the host copy would show (after a
  // solve, an early exit, loadTotalCostMap with an engine) the descents run on the GPU,
  // one lane per path (dymu_extract_paths_device; x, y, z, heading and the counts are
  // bit-identical to the host loop); otherwise -- after
  // propagateGlobalNode, resetTotalCostMap, resetGlobalNarrowBand, or without an
  // engine -- the same host descent runs per start on the host threads.
  // status (optional, one per start): 1 the sink was appended; 0 the descent stalled
  // ("ERROR in trajectory": the waypoints so far are kept); -1 the first step is NaN or
  // the start is off the grid (empty path); -3 more than max_wp waypoints (the first
  // max_wp kept).  stride >= 1 keeps waypoints 0, stride, 2 stride, ... and the sink.
  // sinks (optional, one per start): the goal whose sink waypoint ends the path (0 for a
  // single goal), -1 where status != 1
  std::vector<std::vector<base::Waypoint>> getPaths(const std::vector<base::Waypoint>& starts,
                                                    std::vector<int>* status = nullptr,
                                                    unsigned max_wp = 1u << 20,
                                                    unsigned stride = 1,
                                                    std::vector<int>* sinks = nullptr);
  // Goal sets: several goals at once, each with an optional offset (a
  // cost >= 0 already paid when the route ends there).  Every goal is validated as
  // setGoal validates its one; offsets must be finite and >= 0, as many as the goals or
  // none.  Any failure returns false and changes nothing.  setGoal clears the set.
  // With a set active computeEntireTotalCostMap and computeTotalCostMap run one cold
  // multi-source solve of the whole map (dymu_solve_seeds_device; no early exit, and no
  // windowed reuse unless trackSpeedChanges is on), getPath / computeGlobalPath / getPaths
  // end at the goal the label map names for the cell the path is in, and
  // computeLocalPlanning / repairPath with more than one goal return false / -1.
  // globalGoal(), goalI(), goalJ() report goal 0.
  bool setGoals(const std::vector<base::Waypoint>& goals, const std::vector<double>& offsets = {});
  unsigned goalCount() const {
    return !has_goal_ ? 0u : goals_.empty() ? 1u : (unsigned)goals_.size();
  }
  // The nearest-goal label of every node (ny*nx, row-major): the index of the goal its
  // optimal route drains to, 0xFFFFFFFF (DYMU_LABEL_NONE) for none -- a function of the
  // total-cost map alone (include/dymu_fim.h, dymu_goal_labels_device).  On the device
  // while the device map is current, else by the same rule on the host; cached until
  // the map or the goals change.  goalLabel: the nearest node's label, -1 for none.
  void copyGoalLabels(uint32_t* out);
  int goalLabel(base::Waypoint w);
  uint32_t lastLabelRounds() const { return label_rounds_; }
  // Batched total-cost maps: one map per goal, all on the current speed,
  // solved together in one pass sequence (dymu_solve_batch_device: the maps are planes of
  // one stacked domain) and kept on the device.  Every goal is validated as setGoal
  // validates its one; the speed is synchronised as a solve does.  Needs the device
  // engine: without one it returns false.  Any failure returns false and changes nothing.
  // The batch is state of its own: the goal / goal set, the single total-cost map and what
  // is derived from it (getTotalCostMatrix, getPath, getPaths, the labels), current_path and
  // lastSolveKind() are not touched.  It is dropped by initGlobalLayer, setEngineOptions
  // and the next speed synchronisation that finds a change (batchCount() is then 0 and the
  // accessors below return false).
  bool computeTotalCostMaps(const std::vector<base::Waypoint>& goals);
  unsigned batchCount() const { return (unsigned)batch_goals_.size(); }
  const dymu_stats& lastBatchStats() const { return batch_stats_; }
  // Windowed re-propagation of the batch and of a goal set's map; off by
  // default, and with it off every call behaves as described above.  With it on:
  //  - a speed synchronisation that finds a change keeps the batch and remembers the
  //    changed box; computeTotalCostMaps with the held goals (same cells, same order) then
  //    re-propagates every plane from that box (dymu_update_batch_window_device) when it
  //    covers at most a quarter of the grid, does nothing when no change is pending, and
  //    solves cold otherwise; the batch readers (getTotalCosts, copyBatchTotalCost,
  //    getPathsTo) bring the batch up to date first, so none returns a map of the old speed;
  //  - computeEntireTotalCostMap under a goal set re-propagates the map from the changed
  //    box (dymu_update_seeds_window_device) when the device holds the converged map of
  //    the same goals and offsets, reuses it when nothing changed (lastSolveKind() 1 / 2).
  // initGlobalLayer, setEngineOptions, a changed goal or goal set, loadTotalCostMap,
  // resetTotalCostMap and an early-exit solve forget the goal set's map.  With an engine
  // that lacks the update entries the calls behave as with tracking off.
  void trackSpeedChanges(bool on);
  bool tracksSpeedChanges() const { return track_; }
  // How the last computeTotalCostMaps (or the reader that refreshed the batch) ran:
  // 0 cold solve, 1 windowed re-propagation, 2 batch reused
  int lastBatchSolveKind() const { return batch_kind_; }
  // plane b (ny*nx, row-major) raw (+inf unreachable) or as getTotalCostMatrix (-1)
  bool copyBatchTotalCost(unsigned b, double* out, bool raw);
  // out[b * points.size() + m] = what getTotalCost(points[m]) returns on map b (the
  // offset removed on entry, as getTotalCost does), evaluated on the device
  bool getTotalCosts(const std::vector<base::Waypoint>& points, std::vector<double>& out);
  // computeTotalCostMaps(goals) and getTotalCosts(targets, out) in one call: the
  // goals x targets traverse-cost matrix
  bool costMatrix(const std::vector<base::Waypoint>& goals,
                  const std::vector<base::Waypoint>& targets, std::vector<double>& out);
  // costMatrix with an early exit: same arguments, same output, but the
  // batch solve (dymu_solve_batch_until_device) stops once every cell getTotalCost may
  // read for a target is final in every map -- the matrix is that of costMatrix, the work
  // that of the region the targets span.  Worth it when the targets lie near the goals;
  // with a target at the far end of a map the solve runs about as long as the cold batch
  // and pays for its checks on top (DESIGN.md s5.9 has the measured price).  A target
  // whose cell is unreachable at finite speed makes the solve run to convergence.
  // The stack it leaves is a TRUNCATED batch: batchLevel() is the level up to which its
  // maps are final, batchCount() counts its planes and lastBatchStats() reports the solve.
  // A truncated batch is never read and never reused: getTotalCosts, copyBatchTotalCost
  // and getPathsTo first complete it with the cold solve of the held goals
  // (lastBatchSolveKind() is then 0 and batchLevel() +inf), computeTotalCostMaps with the
  // same goals solves cold with or without trackSpeedChanges, and a synchronised speed
  // change drops it.  Without a device engine, or with an engine that lacks the entry, it
  // returns false and changes nothing.
  bool costMatrixUntil(const std::vector<base::Waypoint>& goals,
                       const std::vector<base::Waypoint>& targets, std::vector<double>& out);
  // +inf for a complete batch and with no batch
  double batchLevel() const { return batch_level_; }
  // Combining the maps of the batch cell by cell on the device (DESIGN.md s5.14;
  // dymu_batch_reduce_device in include/dymu_fim.h defines the fold, its order and its tie
  // rules): op over the listed planes (empty: all, in order), each optionally weighted
  // and offset (empty, or one value per listed plane).  The combined map and, for MAX / MIN,
  // the map of the plane that gave each cell stay on the device; summary describes the
  // combined map (its minimum below +inf, that cell, the cells below +inf).  Like the other
  // batch readers it first completes a truncated batch and, with trackSpeedChanges,
  // re-propagates a pending box.  False, with nothing changed: no batch, no device engine,
  // an engine without the entry, a plane >= batchCount(), list lengths that do not match, a
  // weight not finite or not > 0, an offset negative or not finite.
  enum CombineOp { COMBINE_SUM = 0, COMBINE_MAX = 1, COMBINE_MIN = 2 };
  typedef dymu_reduce_summary CombineSummary;
  bool combineTotalCostMaps(CombineOp op, const std::vector<uint32_t>& planes,
                            const std::vector<double>& weights, const std::vector<double>& offsets,
                            CombineSummary* summary = nullptr);
  // The combined map (ny*nx, row-major) raw (+inf) or as getTotalCostMatrix (-1), and the
  // plane map of the last MAX / MIN (0xFFFFFFFF: a MIN cell no plane reaches).  False once
  // the combined map no longer belongs to the batch: after dropBatch, after any solve or
  // refresh that rewrote the stack (lastBatchSolveKind() 0 or 1), after a new grid or new
  // engine options; copyCombinedPlanes also after a SUM.  A reuse (kind 2) keeps it.
  bool copyCombinedTotalCost(double* out, bool raw);
  bool copyCombinedPlanes(uint32_t* out);
  // The corridor between goals a and b of the batch: the via field T_a + T_b (the cost of
  // the best a-b route through each cell; left as the combined map), D_min its discrete
  // minimum (the a-b traverse cost), bound = D_min * (1.0 + slack), and mask (ny*nx bytes)
  // = 1 where the via field is <= bound -- relative to the field's own minimum, so the
  // corridor is never empty.  False, with nothing written: a or b >= batchCount(), slack
  // negative or not finite, no finite cell in the via field, or what combineTotalCostMaps
  // refuses.
  struct CorridorInfo {
    double D_min;
    uint32_t min_i, min_j;        // a cell that attains it (the lowest row-major one)
    uint64_t count;               // marked cells
    uint32_t i0, j0, i1, j1;      // their inclusive box
    double bound;
  };
  bool viaCorridor(unsigned a, unsigned b, double slack, uint8_t* mask, CorridorInfo* info);
  // Where the listed planes' rovers should meet: the cell that minimises the MAX (minimax:
  // everyone there soonest) or the SUM (least total effort) of their weighted, offset maps,
  // and that value; the lowest row-major cell among equals.  False when no cell is finite.
  // Leaves the combined map as combineTotalCostMaps would.
  bool rendezvous(const std::vector<uint32_t>& planes, const std::vector<double>& weights,
                  const std::vector<double>& offsets, bool minimax, unsigned* i, unsigned* j,
                  double* value);
  // the kernel time (HIP events, ms) of the last combine, 0 before the first
  double lastCombineKernelMs() const { return last_combine_ms_; }
  // getPaths on map b with goal b as the sink (always on the device; sinks are 0).
  // Throws std::invalid_argument for b >= batchCount().
  std::vector<std::vector<base::Waypoint>> getPathsTo(unsigned b,
                                                      const std::vector<base::Waypoint>& starts,
                                                      std::vector<int>* status = nullptr,
                                                      unsigned max_wp = 1u << 20,
                                                      unsigned stride = 1);
  // Per-path summaries: for each start the record of the path getPaths
  // (stride 1) returns -- status, sink, waypoint count, length, last hop, and per sampled
  // field the integral along the path, minimum, maximum and skipped samples, exactly as
  // include/dymu_fim.h defines dymu_path_stat on the grid-local waypoints -- without the
  // waypoints ever being stored or moved.  Field slot 0 is the speed map the solve used
  // (risk inflation included; an obstacle's +inf counts as skipped), slot 1 the caller's
  // optional row-major nx*ny `field` (hazard, clearance, elevation ...).  The route is
  // getPaths': on the device (dymu_path_stats_device) while the device map is current,
  // else -- or with host = true -- the same accumulation inside the host descent on the
  // host threads; the records are bit-identical.  last_hop <= (2 + tau) * global_res
  // tells a descent that arrived from one the reference's NaN rule cut short.
  // Throws std::invalid_argument for max_wp = 0.
  typedef dymu_path_stat PathStats;
  std::vector<PathStats> getPathStats(const std::vector<base::Waypoint>& starts,
                                      unsigned max_wp = 1u << 20, const double* field = nullptr,
                                      bool host = false);
  // ... on map b of the batch with goal b as the sink (always on the device; slot 0 is
  // the speed the batch was solved with).  Throws std::invalid_argument for b >= batchCount().
  std::vector<PathStats> getPathStatsTo(unsigned b, const std::vector<base::Waypoint>& starts,
                                        unsigned max_wp = 1u << 20,
                                        const double* field = nullptr);
  // The arriving descent: paths that pass obstacles and end on the goal's
  // node.  getPaths' descent ends where a cell has an obstacle corner (its direction is NaN
  // there) and jumps to the sink; this one takes the same continuous step wherever that step
  // is valid and a node-to-node step on the total cost wherever it is not, never enters an
  // obstacle node's square, and on a converged map arrives from every start on a finite
  // node (include/dymu_fim.h states the rule with dymu_arrive_stat).  Waypoints, status,
  // max_wp, stride and sinks are getPaths'; status -1 is a start whose node is off the grid,
  // an obstacle or (goal set) without a label.  stats (optional, one per start): the
  // record -- status, sink, waypoints and hops at stride 1, length, T at the start's node.
  // The route is getPaths' (dymu_arrive_paths_device while the device map is current, else
  // the same rule on the host threads; bit-identical).  current_path is not touched.
  typedef dymu_arrive_stat ArriveStats;
  std::vector<std::vector<base::Waypoint>> getArrivingPaths(
      const std::vector<base::Waypoint>& starts, std::vector<int>* status = nullptr,
      unsigned max_wp = 1u << 20, unsigned stride = 1, std::vector<int>* sinks = nullptr,
      std::vector<ArriveStats>* stats = nullptr);
  // ... on map b of the batch with goal b as the sink (always on the device).  Throws
  // std::invalid_argument for b >= batchCount().
  std::vector<std::vector<base::Waypoint>> getArrivingPathsTo(
      unsigned b, const std::vector<base::Waypoint>& starts, std::vector<int>* status = nullptr,
      unsigned max_wp = 1u << 20, unsigned stride = 1, std::vector<ArriveStats>* stats = nullptr);
  // the records alone: no waypoint is stored or moved (host = true: the host route)
  std::vector<ArriveStats> getArrivingStats(const std::vector<base::Waypoint>& starts,
                                            unsigned max_wp = 1u << 20, bool host = false);
  std::vector<ArriveStats> getArrivingStatsTo(unsigned b,
                                              const std::vector<base::Waypoint>& starts,
                                              unsigned max_wp = 1u << 20);
  // getArrivingPaths thinned while the descent runs: of the waypoints
  // walked, only those the rule of csrc/path_simplify.h keeps are stored, moved and
  // returned -- the first, the last, the sink, and enough in between that every dropped
  // waypoint lies within eps (map units, > 0) of the segment between the kept waypoints on
  // either side of it (include/dymu_fim.h states the rule with
  // dymu_arrive_simplified_device).  The bound is one-sided -- dropped waypoints to the
  // polyline, not the polyline to anything: choose eps below the clearance relied on.
  // max_wp bounds the walk as in getArrivingStats (status -3 beyond it).  Every returned
  // waypoint equals its getArrivingPaths(stride 1) twin in all four components; index
  // (optional, one vector per start) gives each one's number in that path.  status, sinks
  // and stats are getArrivingPaths'.  The route is getPaths' (bit-identical either way);
  // on the device the first slot capacity is a guess sized from the grid, and a path that
  // keeps more runs once more with the capacity it reported (lastSimplifiedReruns()).
  // Throws std::invalid_argument for eps not finite or <= 0, or max_wp == 0.
  std::vector<std::vector<base::Waypoint>> getSimplifiedPaths(
      const std::vector<base::Waypoint>& starts, double eps, std::vector<int>* status = nullptr,
      unsigned max_wp = 1u << 20, std::vector<int>* sinks = nullptr,
      std::vector<ArriveStats>* stats = nullptr,
      std::vector<std::vector<uint32_t>>* index = nullptr);
  // ... on map b of the batch with goal b as the sink (always on the device).  Throws
  // std::invalid_argument for b >= batchCount().
  std::vector<std::vector<base::Waypoint>> getSimplifiedPathsTo(
      unsigned b, const std::vector<base::Waypoint>& starts, double eps,
      std::vector<int>* status = nullptr, unsigned max_wp = 1u << 20,
      std::vector<ArriveStats>* stats = nullptr,
      std::vector<std::vector<uint32_t>>* index = nullptr);
  // the paths of the last getSimplifiedPaths[To] that ran a second time on the device
  // because they kept more waypoints than the first slot capacity (0 on the host route),
  // and the bytes of records, counts, slots and indices that call downloaded
  uint64_t lastSimplifiedReruns() const { return last_simplified_reruns_; }
  uint64_t lastSimplifiedBytes() const { return last_simplified_bytes_; }
  // Every cell's node route to the goal at once (include/dymu_fim.h states
  // the definition with dymu_route_out): per cell the goal its route ends on, the hops
  // between axis and diagonal neighbours, the length, and per sampled field the integral
  // along the route, the minimum and the maximum.  The route is the hop of the arriving
  // descent applied at every node -- a chain of grid nodes along which the total cost falls
  // strictly and that cuts no obstacle corner, not the mostly continuous path
  // getArrivingPaths returns; its length is octile (up to 8.2 % above a straight run), and
  // under a goal set its sink can differ from the 4-neighbour label of goalLabel().
  // request.fields: up to DYMU_PATH_FIELDS entries, each the speed map the solve used
  // (nullptr, getPathStats' slot 0) or a caller's row-major nx*ny array.  request.outputs:
  // the maps wanted (kRoute* bits); only they are computed.  The device route is getPaths'
  // (dymu_route_fields_device while the device map is current), else -- or with host = true
  // -- the same definition on the host mirror, the cells in ascending total cost, each from
  // its parent.  Integer outputs, length, vmin and vmax are bit-identical between the two;
  // the integrals add the same terms in another order.  current_path is not touched.
  // Without a goal every cell is without a route.
  enum : uint32_t {
    kRouteSink = 1u, kRouteAxis = 2u, kRouteDiag = 4u, kRouteLength = 8u,
    kRouteIntegral = 16u, kRouteMin = 32u, kRouteMax = 64u, kRouteAll = 127u
  };
  struct RouteRequest {
    uint32_t outputs = kRouteAll;
    std::vector<const double*> fields;
    bool host = false;
  };
  struct RouteFields {  // row-major nx*ny maps; empty where not requested
    std::vector<uint32_t> sink, axis, diag;
    std::vector<double> length;
    std::vector<std::vector<double>> integral, vmin, vmax;  // one per requested field
    uint32_t rounds = 0;  // doubling rounds of the device route (0 on the host)
  };
  RouteFields getRouteFields(const RouteRequest& request);
  // ... on map b of the batch with goal b as the root (always on the device; the speed is
  // the one the batch was solved with).  Throws std::invalid_argument for b >= batchCount().
  RouteFields getRouteFieldsTo(unsigned b, const RouteRequest& request);
  // How much of the map drains through every cell (include/dymu_fim.h
  // states the definition with dymu_usage_out): the upstream side of getRouteFields' forest.
  // Per cell usage, the weight of all cells whose route passes through it (itself included;
  // request.weights, a row-major nx*ny array, or 1 a cell), far, the largest total cost among
  // them, and sink, the goal the route ends on; per goal its catchment, the usage at its
  // root (0 for a dominated goal).  A cell without a route gets 0 / NaN / DYMU_LABEL_NONE.
  // request.outputs: what is wanted (kUsage* bits); only that is computed.  The device route
  // is getRouteFields' (dymu_route_usage_device while the device map is current), else -- or
  // with host = true -- the same definition on the host mirror, the cells in descending
  // total cost, each added into its parent.  The two are equal bit for bit.  current_path is
  // not touched.  Without a goal every cell is without a route and catchment is empty.
  enum : uint32_t {
    kUsageUsage = 1u, kUsageFar = 2u, kUsageSink = 4u, kUsageCatchment = 8u, kUsageAll = 15u
  };
  struct RouteUsageRequest {
    uint32_t outputs = kUsageAll;
    const uint32_t* weights = nullptr;
    bool host = false;
  };
  struct RouteUsage {  // row-major nx*ny maps and one entry per goal; empty where not requested
    std::vector<uint64_t> usage;
    std::vector<double> far;
    std::vector<uint32_t> sink;
    std::vector<uint64_t> catchment;
    uint32_t rounds = 0;  // doubling rounds of the device route (0 on the host)
  };
  RouteUsage getRouteUsage(const RouteUsageRequest& request);
  // ... on map b of the batch with goal b as the root (always on the device).  Throws
  // std::invalid_argument for b >= batchCount().
  RouteUsage getRouteUsageTo(unsigned b, const RouteUsageRequest& request);
  // whether the last getPaths / getPathStats / getArriving* / getRouteFields / getRouteUsage ran on the device, and its kernel time (HIP
  // events, ms)
  bool lastPathsOnDevice() const { return last_paths_device_; }
  double lastPathsKernelMs() const { return last_paths_kernel_ms_; }
  // local-layer inspection: how many global nodes are subdivided (mask: ny*nx
  // bytes, may be null), and one subdivided node's sub-cells (r*r each,
  // row-major) -- false if (i, j) has no local map
  uint64_t localMapMask(uint8_t* mask) const;
  bool localBlock(unsigned i, unsigned j, double* dev, double* tc, double* risk, uint8_t* state,
                  uint8_t* obst) const;
  unsigned resRatio() const { return res_ratio_; }
  // ---- obstacle clearance for the global plan ----
  // The reference keeps a rover away from an obstacle in the local layer only, after a
  // repair (expandRisk / propagateRisk).  This gives the global layer the same notion for
  // the obstacles already on the global map: R = max(1 - d / risk_distance, 0), d the
  // distance (metres, Eikonal on the grid) to the nearest obstacle node, is one more
  // per-cell factor of the speed every global solve runs on,
  //   F = (global_res * cost * (2 + hazard - traff)) * (risk_ratio * R + 1),
  // computed on the device (dymu_clearance_device) at the next speed synchronisation after
  // the setting or the obstacles changed, and mirrored on the host.  Off by default and
  // with either argument 0: then every call packs and launches what it did before.
  // Independent of the constructor's risk_distance / risk_ratio (the local layer's).
  // false, and nothing changes: a negative, NaN or infinite argument; a non-zero setting
  // without a device engine or on an engine that lacks the entry.  A change re-packs the
  // whole map at the next solve.
  bool setGlobalRisk(double risk_distance, double risk_ratio);
  double globalRiskDistance() const { return grisk_distance_; }
  double globalRiskRatio() const { return grisk_ratio_; }
  // R as [j][i] (recomputed first when stale); all zeros while the feature is off
  std::vector<std::vector<double>> getGlobalRiskMatrix();
  // How R was last brought up to date: 0 not yet, 1 the whole clearance solve, 2 the
  // incremental update after setCostMapWindow added obstacles (dymu_clearance_update_device:
  // the box's speed uploaded, the field re-propagated from the new cells, the rows of the
  // box the engine reports downloaded and re-packed), 3 the same after a box that freed
  // obstacles, with or without adding others (trackObstacleRemoval,
  // dymu_clearance_edit_device: the field raised where the freed cells supported it, then
  // re-propagated; R falls as well as rises inside the box).
  int lastRiskUpdateKind() const { return risk_update_kind_; }
  // Off (the default): an obstacle that setCostMapWindow frees sends R through the whole
  // clearance solve.  On: it joins the pending box like an added one, provided the global
  // risk is on, R is current, the resident maps are those R belongs to and the engine has
  // the edit entry; a stale R, dropped maps or an engine error leave the whole solve
  // (kind 1) as before.  Takes effect from the next setCostMapWindow.
  void trackObstacleRemoval(bool on) { track_removal_ = on; }
  bool tracksObstacleRemoval() const { return track_removal_; }
  // ... the engine's statistics of that solve or update (ms: its device time), and the box
  // {i0, j0, w, h} of R it rewrote: the whole grid, or what the incremental update reported
  const dymu_stats& lastRiskStats() const { return risk_stats_; }
  const uint32_t* lastRiskBox() const { return risk_box_; }
  // {raise passes, raise tile visits, cells invalidated, 0} of the last update of kind 3
  // (dymu_last_update_stats); zeros after every other kind
  const uint64_t* lastRiskRaise() const { return risk_raise_; }

 private:
  // the global risk: on iff both are > 0; R (ny*nx, empty while off) belongs to the
  // obstacles and the distance it was computed for, else risk_stale_
  double grisk_distance_ = 0.0, grisk_ratio_ = 0.0;
  std::vector<double> global_risk_;
  bool risk_stale_ = false;
  bool globalRiskOn() const { return grisk_distance_ > 0 && grisk_ratio_ > 0; }
  // the obstacle mask (the raw speed), the constant work map and the clearance field,
  // resident on the device: allocated at the first refresh of a grid, freed where dF_ /
  // dT_ are.  risk_dev_valid_: they are those R was computed from
  double *dMask_ = nullptr, *dW_ = nullptr, *dS_ = nullptr;
  bool risk_dev_valid_ = false;
  void dropRiskMaps();
  // obstacles setCostMapWindow added since R was brought up to date (and, with
  // track_removal_, freed: risk_pend_freed_): their bounding box
  bool risk_pend_ = false, risk_pend_freed_ = false, track_removal_ = false;
  unsigned rpend_i0_ = 0, rpend_i1_ = 0, rpend_j0_ = 0, rpend_j1_ = 0;
  int risk_update_kind_ = 0;
  dymu_stats risk_stats_{};
  uint32_t risk_box_[4] = {0, 0, 0, 0};
  uint64_t risk_raise_[4] = {0, 0, 0, 0};
  // the speed without the risk factor, +inf for an obstacle node: the mask's source
  double rawSpeed(uint64_t k) const {
    return is_obstacle_[k] ? std::numeric_limits<double>::infinity()
                           : global_res_ * cost_[k] * (2 + hazard_[k] - traff_[k]);
  }
  // R up to date: the whole recompute when stale, else the pending box incrementally
  void syncGlobalRisk() {
    if (!globalRiskOn()) return;
    if (risk_stale_) refreshGlobalRisk();
    else if (risk_pend_) updateGlobalRisk();
  }
  void updateGlobalRisk();
  // the speed of a non-obstacle node (:527-528), with the risk factor while that is on:
  // the one expression syncSpeed packs and propagateGlobalNode updates with
  double nodeSpeed(uint64_t k) const {
    const double f = global_res_ * cost_[k] * (2 + hazard_[k] - traff_[k]);
    return global_risk_.empty() ? f : f * (grisk_ratio_ * global_risk_[k] + 1.0);
  }
  // R from the obstacles now on the map: the raw speed and the clearance field on the
  // resident device maps, R = max(1 - S, 0); every row dirty
  void refreshGlobalRisk();
  uint64_t idx(unsigned i, unsigned j) const { return (uint64_t)j * nx_ + i; }
  // total cost of cell k: the device map, fetched into the host mirror in blocks
  // of kBlk x kBlk cells on first read
  double T(uint64_t k) const;
  void fetchAll() const;
  // body(r0, r1) over row chunks of the total cost, each once it is in the host
  // mirror (a stale mirror downloads chunk k+1 while body runs on chunk k)
  template <class Body>
  void streamTotalCost(Body&& body) const;
  // the reference's node state: CLOSED iff popped by its FMM (finite T not above
  // the last early-exit limit; every finite cell after a full solve)
  bool closedCell(uint64_t k) const;
  // node states written by a caller (setGlobalNodeState, resetTotalCostMap): empty =
  // derived from the last solve (closedCell's rule), else 1 = CLOSED per node
  std::vector<uint8_t> node_state_;
  void materializeStates();
  // nodes propagateGlobalNode made finite (global_propagated_nodes beyond the map's)
  std::vector<uint64_t> propagated_extra_;
  bool manual_list_ = false;  // after resetTotalCostMap: the list is propagated_extra_ alone
  // local per-node helpers (csrc/local_layer.cpp)
  void riskUpdate(uint64_t q);
  void deviationUpdate(uint64_t q);
  int64_t localId(const localNode& n) const;
  void markDirty(unsigned j0, unsigned j1);
  void ensureEngine();
  // pack F for the dirty rows, upload the rows whose speed changed; returns false
  // when nothing changed, else the bounding box of the changed cells
  bool syncSpeed(unsigned& i0, unsigned& i1, unsigned& j0, unsigned& j1);
  template <class ERows, class TRows>
  bool costMapFromRows(const ERows& elev_row, const TRows& terr_row);
  bool propagate(bool early, unsigned si, unsigned sj);
  // the band's tentative values at the moment `last` was popped; true when they are
  // not to be used: the reference's pop order was undetermined or near-tied (guard),
  // or the replay hit its work bound
  bool replayBand(uint64_t last, const std::vector<uint64_t>& band, std::vector<double>& out,
                  TieGuard& guard);
  // the reference's early exit replayed exactly on the host over the region box
  // (inclusive; empty: the whole grid) -- when the values cannot decide the exit
  bool exactEarlyExit(unsigned si, unsigned sj, const int64_t box[4]);
  // the reference FMM on the host (exact): until (si, sj) and its nb4 are CLOSED, or
  // the band empties for si < 0; over a box (inclusive, grown to the grid if short)
  struct HostFmm {
    int64_t bx[4], W = 0, PW = 0;
    std::vector<double> T;        // the box with a one-cell ring (+inf), row pitch PW
    std::vector<uint8_t> st;      // 1 CLOSED, 2 in the band (ring: 3 off the box, 4 off the grid)
    uint64_t at(int64_t i, int64_t j) const {  // grid cell (i, j) inside the box
      return (uint64_t)(j - bx[1] + 1) * (uint64_t)PW + (uint64_t)(i - bx[0] + 1);
    }
    std::vector<uint64_t> order;  // grid indices, in first-insertion order
    uint64_t band = 0;
  };
  HostFmm hostFmm(int64_t si, int64_t sj, const int64_t box[4]) const;
  // global_propagated_nodes' order after a GPU solve (reference insertion order)
  std::vector<uint64_t> insertionOrder();
  bool have_start_ = false;  // the last early exit's start and region (exact fallback)
  unsigned start_i_ = 0, start_j_ = 0;
  int64_t exit_box_[4] = {0, 0, -1, -1};
  double exit_r_const_ = 0.0;  // the constant-speed radius around the goal (TieGuard)
  // true once minCostGlobalNode checked the band's values for near ties (or the band
  // is exact / caller-built)
  bool band_values_checked_ = true;
  void settleBand();  // the check, and the exact replay on a near tie
  static constexpr uint64_t kReplayBudget = 1ull << 26;  // band-replay updates per exit
  static constexpr double kTieEps = 1e-12;        // near-tie bound (relative, TieGuard)
  static constexpr double kRegionMargin = 1e-9;   // the exit region: T <= t_closed (1 + this)
  // the host mirror's values for PopOrder
  struct MapT {
    const DyMuPathPlanner* p;
    double operator()(uint64_t k) const { return p->T(k); }
  };
  // band_cells_ into the reference's insertion order, if still in grid order
  void orderBand();
  bool safeNode(unsigned i, unsigned j) const;
  // computeNextGlobalWaypoint / computeGlobalPath without member writes (getPaths'
  // host threads share them): descend returns getPaths' status
  base::Waypoint nextWaypoint(base::Waypoint& wPos, double tau) const;
  // With acc (getPathStats) every waypoint that would be kept joins the record instead
  // of `path`, which stays empty.
  struct PathAccum;
  int descend(base::Waypoint wPos, std::vector<base::Waypoint>& path, uint64_t max_wp,
              unsigned stride, int* sink = nullptr, PathAccum* acc = nullptr) const;
  // target: another device map of this grid and its sink (getPathsTo) in place of dT_
  // and the goal / goal set
  struct PathTarget {
    const double* map;
    unsigned gi, gj;
    double heading;
  };
  // one call of a device descent entry: its map and sinks, uploads and error text
  struct DeviceQuery;
  // the device holds the current map, and the goal set's labels if there is one: the
  // descent entries can run there
  bool descentOnDevice() const;
  // the single sink's waypoint, grid-local: node (gi, gj) with this heading
  base::Waypoint nodeSink(unsigned gi, unsigned gj, double heading) const;
  // arrive: the arriving descent (dymu_arrive_paths_device) in place of the reference's,
  // its records into *arrive
  void pathsOnDevice(const std::vector<base::Waypoint>& starts,
                     std::vector<std::vector<base::Waypoint>>& out, std::vector<int>& st,
                     std::vector<int>& sinks, unsigned max_wp, unsigned stride,
                     const PathTarget* target = nullptr,
                     std::vector<ArriveStats>* arrive = nullptr);
  // getPaths' host post-pass: c slots (x, y, dcx, dcy; grid-local) of a path with this
  // status into waypoints -- z from the elevation, heading from the direction, the
  // offsets added; slot 0 keeps the start's z and heading, a status-1 path ends on `sink`
  void slotsToPath(const double* slots, uint64_t c, int status, const base::Waypoint& start,
                   const base::Waypoint& sink, std::vector<base::Waypoint>& path) const;
  // the arriving descent from grid-local (x, y) on T() (labels_ under a goal set): the
  // kept slots into *slots (null: none stored), the record into rec; returns the status
  // eps (null: none): the walk at stride 1 through the rule of csrc/path_simplify.h --
  // only the waypoints it keeps go to *slots, their numbers in the walk to *index
  int descendArriving(double x, double y, uint64_t max_wp, unsigned stride,
                      std::vector<double>* slots, ArriveStats& rec, const double* eps = nullptr,
                      std::vector<uint32_t>* index = nullptr) const;
  // the device route of getSimplifiedPaths[To]
  void simplifiedOnDevice(const std::vector<base::Waypoint>& starts, double eps,
                          std::vector<std::vector<base::Waypoint>>& out, std::vector<int>& st,
                          std::vector<int>& sinks, unsigned max_wp, const PathTarget* target,
                          std::vector<ArriveStats>& rec,
                          std::vector<std::vector<uint32_t>>* index);
  uint64_t last_simplified_reruns_ = 0, last_simplified_bytes_ = 0;
  void arriveStatsOnDevice(const std::vector<base::Waypoint>& starts,
                           std::vector<ArriveStats>& out, unsigned max_wp,
                           const PathTarget* target);
  void pathStatsOnDevice(const std::vector<base::Waypoint>& starts, std::vector<PathStats>& out,
                         unsigned max_wp, const double* field, const PathTarget* target);
  // getPathStats' copy of the caller's field on the device: dcells_ doubles, allocated on
  // first use and kept until the map buffers go (dropLabels), never re-allocated per call
  double* d_pfield_ = nullptr;
  // getRouteFields on the device: the caller's fields (dcells_ doubles each), the output
  // maps (dcells_ elements each: sink, axis, diag; length; per field integral, vmin, vmax)
  // and the engine's workspace, plain cached device memory.  Each is allocated on first
  // use and kept until the map buffers go (dropLabels); the workspace alone is replaced,
  // when a request needs more than it holds.
  double* d_rfield_[DYMU_PATH_FIELDS] = {};
  uint32_t* d_rout_u_[3] = {};
  double* d_rout_len_ = nullptr;
  double* d_rout_f_[3][DYMU_PATH_FIELDS] = {};
  void* d_route_ws_ = nullptr;
  size_t route_ws_bytes_ = 0;
  void routeFieldsOnDevice(const RouteRequest& rq, const double* map,
                           const std::vector<dymu_seed>& seeds, RouteFields& out);
  void routeFieldsOnHost(const RouteRequest& rq, RouteFields& out);
  // getRouteUsage on the device: the caller's weights (dcells_ uint32), the output maps
  // (usage, far, sink) and the engine's workspace, parked and dropped as the buffers above
  uint32_t* d_uweight_ = nullptr;
  uint64_t* d_uout_usage_ = nullptr;
  double* d_uout_far_ = nullptr;
  uint32_t* d_uout_sink_ = nullptr;
  void* d_usage_ws_ = nullptr;
  size_t usage_ws_bytes_ = 0;
  void routeUsageOnDevice(const RouteUsageRequest& rq, const double* map,
                          const std::vector<dymu_seed>& seeds, RouteUsage& out);
  void routeUsageOnHost(const RouteUsageRequest& rq, RouteUsage& out);
  void dropRouteBuffers();
  // the batch (computeTotalCostMaps): its goals and the solved stack, plane b at
  // dT_batch_ + b * dymu_batch_plane_rows(ny_) * nx_ (pitch nx_)
  struct BatchGoal {
    unsigned i, j;
    double heading;
  };
  std::vector<BatchGoal> batch_goals_;
  double* dT_batch_ = nullptr;
  dymu_stats batch_stats_{};
  // costMatrixUntil's truncated batch: the level up to which its planes are final
  // (+inf: a complete batch, or none)
  double batch_level_ = __builtin_inf();
  void dropBatch();
  // the combined map (combineTotalCostMaps): nx_*ny_ doubles, the arg map and viaCorridor's
  // byte mask, pitch nx_; allocated on first use, kept for the grid (dropCombined frees them
  // where the map buffers go); comb_valid_: the combined map is that of the held stack
  double* d_comb_ = nullptr;
  uint32_t* d_comb_arg_ = nullptr;
  uint8_t* d_comb_mask_ = nullptr;
  bool comb_valid_ = false, comb_arg_valid_ = false;
  double last_combine_ms_ = 0.0;
  void dropCombined();
  // the held batch brought up to date and the reduction run into d_comb_ / d_comb_arg_
  bool combineOnDevice(int op, const std::vector<uint32_t>& planes,
                       const std::vector<double>& weights, const std::vector<double>& offsets,
                       dymu_reduce_summary& s);
  // computeTotalCostMaps' preamble: the goals validated into bg, the engine made, the
  // speed synchronised (a change found is passed on as there); false: rejected
  bool prepareBatch(const std::vector<base::Waypoint>& goals, std::vector<BatchGoal>& bg);
  // getTotalCost of every point on every plane of the held stack, as it stands
  void gatherBatch(const std::vector<base::Waypoint>& points, std::vector<double>& out);
  // goal cell of w by setGoal's tests; false if setGoal would reject it
  bool goalCell(const base::Waypoint& w, unsigned& i, unsigned& j) const;
  // a speed change a batch solve synchronised while dT_ still holds the map of the
  // old speed: its box joins what the next single-goal solve finds changed
  bool pend_ = false, pend_dec_ = true;
  unsigned pend_i0_ = 0, pend_i1_ = 0, pend_j0_ = 0, pend_j1_ = 0;
  // trackSpeedChanges: the same bookkeeping for the batch (the box its planes have not
  // seen yet), and the seed list whose converged map dT_ holds (empty: none)
  bool track_ = false;
  int batch_kind_ = 0;
  bool bpend_ = false, bpend_dec_ = true;
  unsigned bpend_i0_ = 0, bpend_i1_ = 0, bpend_j0_ = 0, bpend_j1_ = 0;
  std::vector<dymu_seed> gs_seeds_;
  // a synchronised change of the box [i0, i1) x [j0, j1): drops the batch, or keeps it
  // with the box pending (tracking on)
  void batchSpeedChanged(unsigned i0, unsigned i1, unsigned j0, unsigned j1);
  // the cold solve of a batch from the current dF_; installs it on success
  bool solveBatchCold(std::vector<BatchGoal>& bg);
  // the held batch brought to the current dF_ (windowed where the pending box allows,
  // else cold); false: it could not be and was dropped
  bool refreshBatch();
  // goal sets: empty = the single goal of setGoal
  struct Goal {
    unsigned i, j;
    double heading, t0;
  };
  std::vector<Goal> goals_;
  std::vector<dymu_seed> seedList() const;      // the goals as engine seeds
  base::Waypoint sinkWaypoint(size_t k) const;  // goal k's sink, grid-local
  bool propagateGoals();                        // the cold multi-source solve
  std::vector<uint64_t> sortedFinite();         // finite cells by (total cost, index)
  bool goalsOnDevice() const;                   // the engine has the goal-set entries
  // label caches: the host copy (labels_) and the device map (d_label_, plain cached
  // device memory of dcells_ words, allocated on first use, freed with the engine)
  std::vector<uint32_t> labels_;
  bool labels_valid_ = false, d_label_valid_ = false;
  uint32_t* d_label_ = nullptr;
  uint32_t label_rounds_ = 0;
  void invalidateLabels() { labels_valid_ = d_label_valid_ = false; }
  void dropLabels();           // ... and free the device map
  void ensureDeviceLabels();   // d_label_ from dT_
  void ensureHostLabels();     // labels_: downloaded, or by the host routine
  // dT_ holds what the host mirror would show: set by the solves, the early exit's
  // scatters and uploads, loadTotalCostMap with an engine; cleared wherever the host
  // copy is written alone
  bool dev_map_current_ = false;
  bool last_paths_device_ = false;
  double last_paths_kernel_ms_ = 0.0;
  std::optional<globalNode> snapshot(uint64_t k);
  void nominalCost(unsigned i, unsigned j, int range, int num_locs, double cmax);
  // local layer internals (csrc/local_layer.cpp)
  int64_t nearestIndex(double x, double y) const;
  uint64_t localCell(uint64_t p, localNode* out) const;
  int64_t localAt(double x, double y);  // getLocalNode by sub-cell id, -1 = NULL
  double localTotalCost(uint64_t p) const;
  bool isBlockingObstacle(uint64_t p, unsigned& maxIndex, unsigned& minIndex,
                          const PathIndex* index = nullptr) const;
  int64_t localPropagation(base::Waypoint wInit, base::Waypoint wOvertake);
  std::vector<base::Waypoint> localPath(uint64_t set, base::Waypoint wInit);
  base::Waypoint dijkstraStep(uint64_t l) const;
  void windowMatrix(base::Waypoint rover_pos, bool deviation, std::vector<std::vector<double>>& m);

  static constexpr unsigned kBlk = 128;

  // parameters (src/DyMu.hpp:399-427)
  double risk_distance_, reconnect_distance_, risk_ratio_;
  repairingAproach repairing_approach_;
  unsigned nx_ = 0, ny_ = 0;
  double global_res_ = 1.0, local_res_ = 1.0;
  double local_timeout_s_ = 5.0;
  int64_t local_agent_ = -1;         // local_agent (sub-cell id), -1 = NULL
  unsigned res_ratio_ = 1;
  std::unique_ptr<LocalLayer> local_;
  std::vector<double> global_offset_{0.0, 0.0};
  std::vector<double> slope_range_;
  std::vector<std::string> locomotion_modes_;

  // SoA node fields (globalNode, src/DyMu.hpp:69-108)
  std::vector<double> elevation_, slope_, raw_cost_, cost_, hazard_, traff_;
  std::vector<uint32_t> terrain_;
  std::vector<uint8_t> is_obstacle_;
  std::vector<int32_t> loc_mode_;  // -1 = "DONT_CARE"

  bool has_goal_ = false;
  unsigned goal_i_ = 0, goal_j_ = 0;
  double goal_heading_ = 0.0;

  // engine and its device-resident map (pitch nx_)
  dymu_ctx* ctx_ = nullptr;
  dymu_opts opts_{-1, 0, 0, 0, 0, 0, 0, 0, 0};
  dymu_stats stats_{};
  double* dF_ = nullptr;
  double* dT_ = nullptr;
  uint64_t dcells_ = 0;
  // host mirror of dT_
  mutable std::vector<double> total_cost_;
  mutable std::vector<uint8_t> blk_ok_;  // read / written with atomic builtins (T())
  mutable uint64_t blk_missing_ = 0;
  mutable std::mutex fetch_mu_;          // T(): one block download at a time
  unsigned nbx_ = 0, nby_ = 0;
  void* registered_ = nullptr;  // total_cost_ buffer page-locked for DMA
  double closed_limit_ = 0.0;   // CLOSED iff finite T <= closed_limit_ ...
  // ... except these cells of exactly closed_limit_ (sorted): the reference's early
  // exit came before it popped them
  std::vector<uint64_t> open_at_limit_;
  std::vector<uint64_t> band_cells_;  // global_narrowband: grid indices
  bool band_unordered_ = false;       // band_cells_ in grid order until orderBand()
  EarlyExitInfo early_info_{};
  // F as uploaded to dF_ (host copy); node-field rows [dirty_j0_, dirty_j1_)
  // changed since it was packed
  std::vector<double> speed_;
  std::vector<double> row_;
  bool speed_valid_ = false;
  bool decrease_only_ = false;  // the last syncSpeed changed no speed upwards
  unsigned dirty_j0_ = 0, dirty_j1_ = 0;
  bool solved_ = false;  // dT_ holds the converged map of speed_ for the goal below
  unsigned solved_gi_ = 0, solved_gj_ = 0;
  int incremental_ = 0;  // last solve: 0 cold, 1 windowed re-propagation, 2 reused
};

}  // namespace PathPlanning_lib
