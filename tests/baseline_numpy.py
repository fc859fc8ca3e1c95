"""The baseline follower of include/ftl.h (ftl_baseline_act) restated in numpy / Python, one env at a time -- the host twin the CPU tests
pin to the reference's recorded controller (tests/golden/baseline_*.npz) and the GPU tests can be read against.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

FTL_BL_EMPTY, FTL_BL_OVERFLOW = 1, 2
RAD2DEG = 180.0 / math.pi
POP_AT = 20.0


def angle_to_point(cx, cy, tx, ty):
    """MISC:16-26 on float64, the operation sequence of ftl_device.hpp."""
    rx, ry = tx - cx, ty - cy
    if rx > 0.0:
        res = math.atan(ry / rx) * RAD2DEG
    elif rx < 0.0:
        res = math.atan(ry / rx) * RAD2DEG + 180.0
    else:
        res = 0.0
    if res >= 360.0:
        return res - 360.0
    if res < 0.0:
        return 360.0 + res
    return res


def euclid_cr(ax, ay, bx, by):
    """The correctly rounded sqrt(dx^2 + dy^2) of the two float64 differences, decided in integers: the floor of the root to 65 bits or
    more, a sticky bit for what lies below, one correctly rounded division."""
    dx, dy = float(ax) - float(bx), float(ay) - float(by)
    (nx, qx), (ny, qy) = dx.as_integer_ratio(), dy.as_integer_ratio()
    q = max(qx, qy)                      # powers of two
    s = (nx * (q // qx)) ** 2 + (ny * (q // qy)) ** 2          # the sum of squares is s / q^2
    if s == 0:
        return 0.0
    k = max(0, 130 - s.bit_length())
    k += k & 1
    r = math.isqrt(s << k)
    r = (r << 1) | (r * r != s << k)
    return r / ((1 << (k // 2 + 1)) * q)


def euclid_x87(ax, ay, bx, by):
    """BLAS dnrm2 as the reference's scipy runs it (oracle/ftl_oracle.c, numeric notes): the float64 differences squared and summed in the
    x87 64-bit mantissa, sqrtl, one more rounding to float64."""
    dx, dy = np.longdouble(float(ax) - float(bx)), np.longdouble(float(ay) - float(by))
    return float(np.sqrt(dx * dx + dy * dy))


def turn(desirable, cur):
    """(delta_turn, sign) by the four branches of MISC:73-91."""
    if desirable - cur > 0:
        if desirable - cur > 180:
            return cur + (360 - desirable), -1
        return desirable - cur, 1
    if desirable - cur < 0:
        if cur - desirable > 180:
            return (360 - cur) + desirable, 1
        return cur - desirable, -1
    return 0, 0


def move_to_the_point(direction, pos, point, euclid=euclid_cr):
    """(v, w) of MISC:65-95 for a float32 direction, a float32 position pair and a float64 point."""
    px, py = float(np.float32(pos[0])), float(np.float32(pos[1]))
    desirable = int(angle_to_point(px, py, float(point[0]), float(point[1])))
    delta, sign = turn(desirable, int(np.float32(direction)))
    return euclid(px, py, float(point[0]), float(point[1])), float(delta * sign) / 10.0


class Follower:
    """One follower row: the FIFO as a list (front first), the pending pop, the sticky flags."""

    def __init__(self, cap=64):
        self.cap, self.fifo, self.pending, self.flags = cap, [], False, 0
        self.appended = self.popped = False          # what the last act() booked for the step before it

    def act(self, num, target, step_count):
        """``num``: the env's obs_num row, ``target``: its float64 target pair, ``step_count``: its FTL_EI_STEP_COUNT word."""
        t = (float(target[0]), float(target[1]))
        self.appended = self.popped = False
        if step_count == 0 or not self.fifo:
            self.fifo = [t]
        else:
            back = self.fifo[-1]
            if t[0] != back[0] or t[1] != back[1]:
                if len(self.fifo) == self.cap:
                    self.fifo.pop(0)
                    self.flags |= FTL_BL_OVERFLOW
                self.fifo.append(t)
                self.appended = True
            if self.pending:
                if len(self.fifo) > 1:
                    self.fifo.pop(0)
                    self.popped = True
                else:
                    self.flags |= FTL_BL_EMPTY
        v, w = move_to_the_point(num[8], (num[5], num[6]), self.fifo[0])
        self.pending = v <= POP_AT
        return v, w
