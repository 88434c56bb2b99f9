"""Sequential NumPy restatement of PoseGraph::optimize4DoF (pose_graph.cpp:403-579) over several sequences, as
vpl_pg_optimize_seq_batch runs it: tests/pg_ref.py's minimiser, small maths and linear algebra, with the rules the `sequence` of
every node brings (pose_graph.cpp:447-519).

- A node is constant if it is local node 0 or its sequence is 0; sequence=None means every node is of sequence 1.
- The sequential edge (i, i-j), j = 1..4, exists only between two nodes of one sequence.
- An edge, sequential or loop, whose two ends are both constant is not part of the problem: no cost, no gradient, no tolerance
  test (ceres drops it from the reduced program; its fixed cost is NOT added back here, so the costs are the minimiser's).
- A free node that no remaining edge touches is not part of the problem either (ceres drops an unused parameter block): it is
  treated as constant.
- x_norm, the step norm and gmax run over the free nodes.  A constant node keeps its incoming T.

Every node keeps its slot in the linear system, as on the device: a constant node has zero Jacobian blocks, Jacobi scale 1 and a
unit diagonal, so its step is zero.  On a graph of one non-zero sequence every operation is pg_ref.optimize's, in its order."""
import numpy as np

import pg_ref
from pg_ref import (BW, CONVERGENCE, FAILURE, NO_CONVERGENCE, OK, R2ypr, default_options, edge_eval, huber, mat2q, norm_angle, qmat,
                    solve_system, ypr2R)

INVALID = -1


def node_plan(n, loop_local, sequence):
    """-> (const [n] bool, edges [(a, b, loop)] in the order of pg_ref.build_edges without the masked ones)"""
    seq = np.ones(n, dtype=np.int64) if sequence is None else np.asarray(sequence, dtype=np.int64)
    const0 = np.array([k == 0 or seq[k] == 0 for k in range(n)], dtype=bool)
    edges = []
    for i in range(1, n):
        for j in range(1, BW + 1):
            if i - j >= 0 and seq[i] == seq[i - j] and not (const0[i] and const0[i - j]):
                edges.append((i - j, i, False))
    for i in range(n):
        a = int(loop_local[i])
        if a >= 0 and not (const0[i] and const0[a]):
            edges.append((a, i, True))
    touched = np.zeros(n, dtype=bool)
    for a, b, _ in edges:
        touched[a] = touched[b] = True
    return const0 | ~touched, edges


def optimize(vio_T, vio_R, loop_local, loop_info, sequence=None, tail_T=None, tail_R=None, opt=None, dtype=np.float64, solver="banded"):
    dt = dtype
    o = dict(default_options())
    o.update(opt or {})
    n = len(vio_T)
    vio_T = np.asarray(vio_T, dtype=np.float64).reshape(n, 3).astype(dt)
    vio_R = np.asarray(vio_R, dtype=np.float64).reshape(n, 3, 3).astype(dt)
    loop_local = np.asarray(loop_local, dtype=np.int64)
    loop_info = np.asarray(loop_info, dtype=np.float64).reshape(n, 8).astype(dt)
    if sequence is not None and (np.asarray(sequence) < 0).any():
        return dict(status=INVALID)
    assert all(loop_local[i] < i for i in range(n))
    P = {k: (dt(v) if isinstance(v, float) else v) for k, v in o.items()}
    Rq = [qmat(mat2q(vio_R[k])) for k in range(n)]
    eul = [R2ypr(Rq[k]) for k in range(n)]
    x = np.array([[eul[k][0], *vio_T[k]] for k in range(n)], dtype=dt)
    pr = np.array([[eul[k][1], eul[k][2]] for k in range(n)], dtype=dt)
    const, edges = node_plan(n, loop_local, sequence)
    free = np.flatnonzero(~const)
    meas = np.zeros((len(edges), 4), dtype=dt)
    for e, (a, b, loop) in enumerate(edges):
        if loop:
            meas[e, :3], meas[e, 3] = loop_info[b, :3], loop_info[b, 7]
        else:
            meas[e, :3] = Rq[a].T.dot(vio_T[b] - vio_T[a])
            meas[e, 3] = eul[b][0] - eul[a][0]
    m = 4 * (n - 1)
    const_rows = np.repeat(const[1:], 4)
    decisions, rhos, verdicts = [], [], []
    res = dict(status=OK, termination=CONVERGENCE, iterations=0, successful_steps=0, unsuccessful_steps=0, initial_cost=dt(0), final_cost=dt(0),
               decisions=decisions, rhos=rhos, verdicts=verdicts, first=None, edges=edges, const=const)

    def evaluate(xs, jac):
        E = len(edges)
        r, Ja, Jb, cost = np.zeros((E, 4), dtype=dt), np.zeros((E, 4, 4), dtype=dt), np.zeros((E, 4, 4), dtype=dt), np.zeros(E, dtype=dt)
        for e, (a, b, loop) in enumerate(edges):
            re, ja, jb = edge_eval(xs[a], xs[b], pr[a], meas[e], P["loop_yaw_scale"] if loop else dt(1), jac, decisions)
            sq = re.dot(re)
            rho0, rho1 = sq, dt(1)
            if loop and P["huber_delta"] > 0:
                decisions.append((sq, P["huber_delta"] * P["huber_delta"]))
                rho0, rho1 = huber(sq, P["huber_delta"])
            cost[e] = dt(0.5) * rho0
            if jac:
                sc = np.sqrt(rho1)
                r[e], Ja[e], Jb[e] = re * sc, ja * sc, jb * sc
                if const[a]:
                    Ja[e] = dt(0)
                if const[b]:
                    Jb[e] = dt(0)
        return r, Ja, Jb, cost

    def fixed_sum(v):
        s = dt(0)
        for a in v:
            s += a
        return s

    def gather(r, Ja, Jb):
        g, cn = np.zeros(m, dtype=dt), np.zeros(m, dtype=dt)
        for e, (a, b, loop) in enumerate(edges):
            for node, J in ((a, Ja[e]), (b, Jb[e])):
                if node >= 1:
                    g[4 * (node - 1):4 * node] += J.T.dot(r[e])
                    cn[4 * (node - 1):4 * node] += (J * J).sum(axis=0)
        return g, cn

    def plus(xs, delta):
        out = xs.copy()
        for k in free:
            out[k, 0] = norm_angle(xs[k, 0] + delta[4 * (k - 1)])
            out[k, 1:] = xs[k, 1:] + delta[4 * (k - 1) + 1:4 * k]
        return out

    def gmax_of(xs, g):
        if not len(free):
            return dt(0)
        return np.abs(xs[free].reshape(-1) - plus(xs, -g)[free].reshape(-1)).max()

    if n > 1:
        r, Ja, Jb, cost = evaluate(x, True)
        x_cost = fixed_sum(cost)
        res["initial_cost"] = x_cost
        g, cn = gather(r, Ja, Jb)
        scale = dt(1) / (dt(1) + np.sqrt(cn))
        x_norm = np.sqrt((x[free] * x[free]).sum())
        gmax = gmax_of(x, g)
        radius, decrease = P["initial_radius"], dt(2)
        iteration, last_ok, invalid = 0, True, 0
        while True:
            if last_ok:
                res["successful_steps"] += 1
            else:
                res["unsuccessful_steps"] += 1
            if iteration >= o["max_iterations"]:
                res["termination"] = NO_CONVERGENCE
                break
            if last_ok:
                decisions.append((gmax, P["gradient_tolerance"]))
                if gmax <= P["gradient_tolerance"]:
                    break
            decisions.append((radius, P["min_radius"]))
            if radius <= P["min_radius"]:
                break
            iteration += 1
            diag = np.minimum(np.maximum(scale * scale * cn, P["min_lm_diagonal"]), P["max_lm_diagonal"]) / radius
            diag[const_rows] = dt(1)
            y = solve_system(m, edges, Ja, Jb, r, scale, diag, solver)
            valid = y is not None
            if valid:
                delta = -y * scale
                mc = dt(0)
                for e, (a, b, loop) in enumerate(edges):
                    me = Jb[e].dot(delta[4 * (b - 1):4 * b])
                    if a >= 1:
                        me = Ja[e].dot(delta[4 * (a - 1):4 * a]) + me
                    mc += (me * (r[e] + me / dt(2))).sum()
                model = -mc
                if res["first"] is None:
                    res["first"] = dict(g=g.copy(), step=delta.copy(), model=model)
                valid = bool(model > 0)
            if not valid:
                invalid += 1
                verdicts.append("invalid")
                if invalid >= o["max_consecutive_invalid_steps"]:
                    res["termination"] = FAILURE
                    break
                last_ok = False
                continue
            invalid = 0
            cand = plus(x, delta)
            cand_cost = fixed_sum(evaluate(cand, False)[3])
            if not np.isfinite(cand).all() or not np.isfinite(cand_cost):
                cand_cost = dt(np.finfo(np.float64).max)
            d = (x[free] - cand[free]).reshape(-1)
            step_norm = np.sqrt(d.dot(d))
            decisions.append((step_norm, P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"])))
            if step_norm <= P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"]):
                verdicts.append("parameter_tolerance")
                break
            cc = x_cost - cand_cost
            decisions.append((abs(cc), P["function_tolerance"] * x_cost))
            if abs(cc) <= P["function_tolerance"] * x_cost:
                verdicts.append("function_tolerance")
                break
            rho = cc / model
            rhos.append(rho)
            decisions.append((rho, P["min_relative_decrease"]))
            if rho > P["min_relative_decrease"]:
                verdicts.append("accept")
                x, x_cost = cand, cand_cost
                x_norm = np.sqrt((x[free] * x[free]).sum())
                r, Ja, Jb, cost = evaluate(x, True)
                g, cn = gather(r, Ja, Jb)
                gmax = gmax_of(x, g)
                last_ok = True
                t = dt(2) * rho - dt(1)
                radius = min(P["max_radius"], radius / max(dt(1) / dt(3), dt(1) - t * t * t))
                decrease = dt(2)
            else:
                verdicts.append("reject")
                last_ok = False
                radius = radius / decrease
                decrease = decrease * dt(2)
        res["iterations"] = iteration
        res["final_cost"] = x_cost
    res["x"] = x
    res["T"] = x[:, 1:].copy()
    res["R"] = np.array([ypr2R(np.array([x[k, 0], pr[k, 0], pr[k, 1]], dtype=dt)) for k in range(n)], dtype=dt)
    yaw_drift = R2ypr(res["R"][n - 1])[0] - R2ypr(vio_R[n - 1])[0]
    rd = ypr2R(np.array([yaw_drift, dt(0), dt(0)], dtype=dt))
    td = res["T"][n - 1] - rd.dot(vio_T[n - 1])
    res.update(yaw_drift=yaw_drift, r_drift=rd, t_drift=td)
    if tail_T is not None and len(tail_T):
        tT = np.asarray(tail_T, dtype=np.float64).reshape(-1, 3).astype(dt)
        tR = np.asarray(tail_R, dtype=np.float64).reshape(-1, 3, 3).astype(dt)
        res["tail_T"] = np.array([rd.dot(p) + td for p in tT], dtype=dt)
        res["tail_R"] = np.array([rd.dot(Rm) for Rm in tR], dtype=dt)
    return res


solution = pg_ref.solution

MAX_NODES, MAX_LOOPS = 4096, 256
NOTHING = 2


def quat_R(q):
    """the rotation of the quaternion (w, x, y, z) as loop_info carries it, not normalised"""
    return qmat(np.asarray(q))


class PoseGraph:
    """A plain restatement of PoseGraph's list handling -- addKeyFrame (pose_graph.cpp:42-136), loadKeyFrame (:213-287), one turn
    of optimize4DoF's loop body (:407-573), updateKeyFrameLoop (:889-922) -- as vpl_pgs_* runs it: the caller's findConnection has
    already decided, loop_index is its outcome.  Generic in the dtype.  A refused step returns its code and changes nothing."""

    def __init__(self, max_keyframes=8192, fast_relocalization=False, opt=None, dtype=np.float64):
        self.dt, self.cap, self.fast, self.opt = dtype, max_keyframes, fast_relocalization, dict(opt or {})
        self.reset()

    def reset(self):
        dt = self.dt
        self.sequence_cnt, self.sequence_loop, self.earliest_loop_index, self.queue = 0, [0], -1, []
        self.w_r_vio, self.w_t_vio = np.eye(3, dtype=dt), np.zeros(3, dtype=dt)
        self.r_drift, self.t_drift, self.yaw_drift = np.eye(3, dtype=dt), np.zeros(3, dtype=dt), dt(0)
        self.seq, self.loop_index, self.vio_T, self.vio_R, self.T, self.R, self.loop_info = [], [], [], [], [], [], []

    def __len__(self):
        return len(self.seq)

    def _shift(self, oP, oR, info, P, R):
        dt = self.dt
        wP = oR.dot(info[:3]) + oP
        wR = oR.dot(quat_R(info[3:7]))
        yaw = R2ypr(wR)[0] - R2ypr(R)[0]
        return yaw, ypr2R(np.array([yaw, dt(0), dt(0)], dtype=dt)), wP - wR.dot(R.T).dot(P)

    def _note_loop(self, index, loop_index):
        if loop_index >= 0:
            if self.earliest_loop_index > loop_index or self.earliest_loop_index == -1:
                self.earliest_loop_index = loop_index
            self.queue.append(index)

    def _record(self, index):
        return dict(index=index, optimize_pending=bool(self.queue), vio_T=self.vio_T[index].copy(), vio_R=self.vio_R[index].copy(),
                    T=self.T[index].copy(), R=self.R[index].copy(), w_r_vio=self.w_r_vio.copy(), w_t_vio=self.w_t_vio.copy())

    def add(self, sequence, vio_T, vio_R, loop_index=-1, loop_info=None):
        dt = self.dt
        if sequence < 1 or sequence not in (self.sequence_cnt, self.sequence_cnt + 1) or not -1 <= loop_index < len(self):
            return -1
        if len(self) >= self.cap:
            return -4
        if sequence != self.sequence_cnt:
            self.sequence_cnt += 1
            self.sequence_loop.append(0)
            self.w_r_vio, self.w_t_vio = np.eye(3, dtype=dt), np.zeros(3, dtype=dt)
            self.r_drift, self.t_drift = np.eye(3, dtype=dt), np.zeros(3, dtype=dt)
        P = self.w_r_vio.dot(np.asarray(vio_T, np.float64).astype(dt)) + self.w_t_vio
        R = self.w_r_vio.dot(np.asarray(vio_R, np.float64).reshape(3, 3).astype(dt))
        index = len(self)
        info = np.zeros(8, dtype=dt) if loop_index < 0 else np.asarray(loop_info, np.float64).astype(dt)
        if loop_index >= 0:
            if self.seq[loop_index] != sequence and self.sequence_loop[sequence] == 0:
                _, shift_r, shift_t = self._shift(self.vio_T[loop_index], self.vio_R[loop_index], info, P, R)
                self.w_r_vio, self.w_t_vio = shift_r, shift_t
                P, R = shift_r.dot(P) + shift_t, shift_r.dot(R)
                for k in range(index):
                    if self.seq[k] == sequence:
                        self.vio_T[k], self.vio_R[k] = shift_r.dot(self.vio_T[k]) + shift_t, shift_r.dot(self.vio_R[k])
                self.sequence_loop[sequence] = 1
            self._note_loop(index, loop_index)
        self.seq.append(sequence), self.loop_index.append(loop_index), self.loop_info.append(info)
        self.vio_T.append(P), self.vio_R.append(R)
        self.T.append(self.r_drift.dot(P) + self.t_drift), self.R.append(self.r_drift.dot(R))
        return self._record(index)

    def load(self, vio_T, vio_R, T, R, loop_index=-1, loop_info=None):
        dt = self.dt
        if not -1 <= loop_index < len(self):
            return -1
        if len(self) >= self.cap:
            return -4
        index = len(self)
        self._note_loop(index, loop_index)
        self.seq.append(0), self.loop_index.append(loop_index)
        self.loop_info.append(np.zeros(8, dtype=dt) if loop_index < 0 else np.asarray(loop_info, np.float64).astype(dt))
        self.vio_T.append(np.asarray(vio_T, np.float64).astype(dt)), self.vio_R.append(np.asarray(vio_R, np.float64).reshape(3, 3).astype(dt))
        self.T.append(np.asarray(T, np.float64).astype(dt)), self.R.append(np.asarray(R, np.float64).reshape(3, 3).astype(dt))
        return self._record(index)

    def graph(self):
        """the graph the next optimize() runs, as the arguments of optimize(): None when nothing is queued"""
        if not self.queue:
            return None
        first, cur = self.earliest_loop_index, self.queue[-1]
        ks = range(first, cur + 1)
        return dict(first=first, cur=cur, vio_T=np.array([self.vio_T[k] for k in ks]), vio_R=np.array([self.vio_R[k] for k in ks]),
                    loop_local=np.array([self.loop_index[k] - first if self.loop_index[k] >= 0 else -1 for k in ks]),
                    loop_info=np.array([self.loop_info[k] for k in ks]), sequence=np.array([self.seq[k] for k in ks]))

    def optimize(self, solver="banded"):
        g = self.graph()
        if g is None:
            return dict(status=NOTHING)
        if len(g["vio_T"]) > MAX_NODES or (g["loop_local"] >= 0).sum() > MAX_LOOPS:
            return -4
        self.queue = []
        first, cur = g["first"], g["cur"]
        r = optimize(g["vio_T"], g["vio_R"], g["loop_local"], g["loop_info"], g["sequence"], opt=self.opt, dtype=self.dt, solver=solver)
        for i, k in enumerate(range(first, cur + 1)):
            self.T[k], self.R[k] = r["T"][i].copy(), r["R"][i].copy()
        self.yaw_drift, self.r_drift, self.t_drift = r["yaw_drift"], r["r_drift"], r["t_drift"]
        for k in range(cur + 1, len(self)):
            self.T[k], self.R[k] = self.r_drift.dot(self.vio_T[k]) + self.t_drift, self.r_drift.dot(self.vio_R[k])
        r.update(n_nodes=cur - first + 1, first_index=first, cur_index=cur)
        return r

    def update_loop(self, index, loop_info):
        if not 0 <= index < len(self) or self.loop_index[index] < 0:
            return -1
        info = np.asarray(loop_info, np.float64).astype(self.dt)
        if not (abs(info[7]) < 30.0 and np.sqrt(info[:3].dot(info[:3])) < 20.0):
            return False
        self.loop_info[index] = info
        if self.fast:
            old = self.loop_index[index]
            self.yaw_drift, self.r_drift, self.t_drift = self._shift(self.T[old], self.R[old], info, self.vio_T[index], self.vio_R[index])
        return True

    def path(self):
        return dict(T=np.array(self.T).reshape(-1, 3), R=np.array(self.R).reshape(-1, 3, 3), vio_T=np.array(self.vio_T).reshape(-1, 3),
                    vio_R=np.array(self.vio_R).reshape(-1, 3, 3), loop_info=np.array(self.loop_info).reshape(-1, 8),
                    sequence=np.array(self.seq, dtype=np.int32), loop_index=np.array(self.loop_index, dtype=np.int32))
