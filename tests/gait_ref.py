"""The rule of bg_gait_step (csrc/bg_sim.hip) in numpy, sums in float64: a helper of tests/test_gait_metrics.py and tests/test_gpu_gait_metrics.py,
not a test.  It has the form of `Restatement` in tests/test_gpu_evaluate.py: beside every sum it keeps sum|terms| and the number of terms, for the
bound 2 (terms + 12) 2^-24 sum|terms| of an fp32 running sum (terms - 1 roundings of the sum, at most 12 of a term's own: 12 products and 11 adds).

The inputs of step() are the values the env has stored, as T1.get_field returns them (float32), and `clr`, each foot's clearance p.z - ground(p.xy),
which the caller works out (float64; p.z itself on a plane).  Comparisons that the kernel makes on float32 values (contact > 0.5, |cmd| > 1e-6) are
made on float32 here; the slip's d <= 0.5 is made on the float64 distance, so a test keeps its displacements away from half a metre."""
import numpy as np


class GaitRestatement:
    def __init__(self, n):
        from booster_gym_amd import _lib as L

        self.L, self.n = L, n
        self.rec = np.zeros((L.GAIT_PLANES, n))
        self.mag = np.zeros((L.GAIT_PLANES, n))
        self.terms = np.zeros((L.GAIT_PLANES, n))
        self.clr32 = np.zeros((2, n), dtype=np.float32)  # CLR summed in float32 in the kernel's order: bit-equal where the terms are exact
        self.slip_skipped = np.zeros((2, n), dtype=np.int64)  # stance displacements above 0.5 m (the teleport guard)
        self.touchdowns = []  # (len, env, foot, swing steps) of every counted touchdown that closed a swing

    def _add(self, plane, who, values):
        self.rec[plane, who] += values
        self.mag[plane, who] += np.abs(values)
        self.terms[plane, who] += 1

    def begin(self):
        for a in (self.rec, self.mag, self.terms, self.clr32, self.slip_skipped):
            a[:] = 0
        self.touchdowns = []

    def step(self, done, actions, torques, gravity, ang_vel, commands, contact, forces, feet_pos, clr, settle_steps):
        """done [n] bool; actions, torques [n, 12]; gravity, ang_vel, commands [n, 3]; contact [n, 2]; forces, feet_pos [n, 6]; clr [n, 2]."""
        L, r, f64 = self.L, self.rec, np.float64
        FP = L.gait_foot_plane
        run = r[L.GAIT_STATE] == 0                                            # 1
        r[L.GAIT_LEN, run] += 1                                               # 2
        r[L.GAIT_STATE, run & done] = 1                                       # 3
        live = run & ~done
        length = r[L.GAIT_LEN]
        a, tau, g, w = actions.astype(f64), torques.astype(f64), gravity.astype(f64), ang_vel.astype(f64)
        fz, pos, clr = forces.astype(f64)[:, [2, 5]], feet_pos.astype(f64), np.asarray(clr, dtype=f64)
        c = contact > np.float32(0.5)
        self._add(L.GAIT_TAU2, live, (tau ** 2).sum(axis=1)[live])            # 4
        self._add(L.GAIT_TILT, live, (g[:, 0] ** 2 + g[:, 1] ** 2)[live])
        self._add(L.GAIT_WOBBLE, live, (w[:, 0] ** 2 + w[:, 1] ** 2)[live])
        for f in range(2):
            p = FP(L.GAIT_PEAK, f)
            r[p, live] = np.maximum(r[p, live], fz[live, f])
        a1, a2 = r[L.GAIT_A1 : L.GAIT_A1 + 12].T, r[L.GAIT_A2 : L.GAIT_A2 + 12].T
        who = live & (length >= 2)                                            # 5
        self._add(L.GAIT_D1, who, ((a - a1) ** 2).sum(axis=1)[who])
        who = live & (length >= 3)                                            # 6
        self._add(L.GAIT_D2, who, ((a - 2 * a1 + a2) ** 2).sum(axis=1)[who])
        for f in range(2):                                                    # 7
            sw = live & ~c[:, f]
            smax, swn = r[L.GAIT_SWMAX + f], r[L.GAIT_SWN + f]
            smax[sw] = np.where(swn[sw] == 0, clr[sw, f], np.maximum(smax[sw], clr[sw, f]))
            swn[sw] += 1
        m = np.abs(commands).max(axis=1)  # float32, compared as the kernel compares
        moving = live & (length > settle_steps) & (m > np.float32(1e-6))      # 8
        r[L.GAIT_MOV, moving] += 1
        r[L.GAIT_DS, moving & c[:, 0] & c[:, 1]] += 1
        r[L.GAIT_FL, moving & ~c[:, 0] & ~c[:, 1]] += 1
        for f in range(2):
            cprev = r[L.GAIT_CPREV + f] != 0
            r[FP(L.GAIT_STANCE, f), moving & c[:, f]] += 1
            td = moving & (length >= 2) & c[:, f] & ~cprev
            r[FP(L.GAIT_TD, f), td] += 1
            self._add(FP(L.GAIT_IMP, f), td, fz[td, f])
            closed = td & (r[L.GAIT_SWN + f] > 0)
            self._add(FP(L.GAIT_CLR, f), closed, r[L.GAIT_SWMAX + f][closed])
            self.clr32[f, closed] = self.clr32[f, closed] + r[L.GAIT_SWMAX + f][closed].astype(np.float32)
            r[FP(L.GAIT_SWT, f), closed] += r[L.GAIT_SWN + f][closed]
            r[FP(L.GAIT_SWC, f), closed] += 1
            self.touchdowns += [(int(length[e]), int(e), f, int(r[L.GAIT_SWN + f, e])) for e in np.nonzero(closed)[0]]
            st = moving & (length >= 2) & c[:, f] & cprev
            d = np.hypot(pos[:, 3 * f] - r[L.GAIT_PPREV + 2 * f], pos[:, 3 * f + 1] - r[L.GAIT_PPREV + 2 * f + 1])
            self._add(FP(L.GAIT_SLIP, f), st & (d <= 0.5), d[st & (d <= 0.5)])
            self.slip_skipped[f, st & (d > 0.5)] += 1
        for f in range(2):                                                    # 9
            land = live & c[:, f]
            r[L.GAIT_SWN + f, land] = 0
            r[L.GAIT_SWMAX + f, land] = 0
        r[L.GAIT_A2 : L.GAIT_A2 + 12, live] = r[L.GAIT_A1 : L.GAIT_A1 + 12, live]  # 10
        r[L.GAIT_A1 : L.GAIT_A1 + 12, live] = a.T[:, live]
        for f in range(2):
            r[L.GAIT_CPREV + f, live] = c[live, f]
            r[L.GAIT_PPREV + 2 * f, live], r[L.GAIT_PPREV + 2 * f + 1, live] = pos[live, 3 * f], pos[live, 3 * f + 1]

    def planes(self):
        """(exact planes, fp32 running sums, CLR planes, SWMAX planes)."""
        L, FP = self.L, self.L.gait_foot_plane
        feet = lambda k: [FP(k, 0), FP(k, 1)]
        exact = [L.GAIT_STATE, L.GAIT_LEN, L.GAIT_MOV, L.GAIT_DS, L.GAIT_FL] + feet(L.GAIT_STANCE) + feet(L.GAIT_TD) + feet(L.GAIT_SWT) + \
            feet(L.GAIT_SWC) + feet(L.GAIT_PEAK) + list(range(L.GAIT_A1, L.GAIT_PPREV + 4)) + [L.GAIT_SWN, L.GAIT_SWN + 1]
        sums = [L.GAIT_D1, L.GAIT_D2, L.GAIT_TAU2, L.GAIT_TILT, L.GAIT_WOBBLE] + feet(L.GAIT_IMP) + feet(L.GAIT_SLIP)
        clr, swmax = feet(L.GAIT_CLR), [L.GAIT_SWMAX, L.GAIT_SWMAX + 1]
        assert sorted(exact + sums + clr + swmax) == list(range(L.GAIT_PLANES))
        return exact, sums, clr, swmax

    def compare(self, got, where, height_slack=0.0):
        """got: the kernel's record [GAIT_PLANES][n], float32.  height_slack: what a clearance may differ by (0 on a plane: SWMAX and CLR are then
        exact, CLR against the float32 sum of the same terms in the same order; on a height field each term of CLR and SWMAX itself get it on top
        of the running sum's bound).  Returns the worst error / bound of the bounded planes."""
        exact, sums, clr, swmax = self.planes()
        got64 = got.astype(np.float64)
        for p in exact:  # (float32 values in both: equal here is bit-equal)
            assert np.array_equal(got64[p], self.rec[p]), (where, "plane", p, np.nonzero(got64[p] != self.rec[p])[0][:8])
        worst = 0.0

        def bounded(p, bound):
            nonlocal worst
            err = np.abs(got64[p] - self.rec[p])
            assert np.all(err <= bound), (where, "plane", p, int(err.argmax()), float(err.max()), float(bound[err.argmax()]))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))

        for p in sums:
            bounded(p, 2.0 * (self.terms[p] + 12.0) * 2.0 ** -24 * self.mag[p])
        if height_slack == 0.0:
            for f in range(2):
                assert np.array_equal(got64[swmax[f]], self.rec[swmax[f]]), (where, "SWMAX", f)
                assert np.array_equal(got[clr[f]], self.clr32[f]), (where, "CLR", f)
        else:
            for f in range(2):
                bounded(swmax[f], np.full(self.n, height_slack))
                bounded(clr[f], 2.0 * (self.terms[clr[f]] + 12.0) * 2.0 ** -24 * self.mag[clr[f]] + height_slack * self.terms[clr[f]])
        return worst
