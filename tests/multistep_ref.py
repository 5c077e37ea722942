"""References of the multistep (Adams-Bashforth 2 / 3) solvers - the reference project has none, so the definition lives here.

table_loop64         the table-driven loop in fp64 for a scalar ODE dx/dsigma = f(sigma, x): what the device does with a coefficient
                     table of host/tables.solver_table(multistep_order=), without its roundings.
rk4_reference        the same ODE by classical Runge-Kutta in fp64 (the order tests' truth).
The model loop with a velocity history is loop_ref.restated_loop(order= / weights=); the per-element reference of one step with a
history ring is opcheck.step_ref_and_bounds(..., ring, it).
"""
import math

from opcheck import STEP_HIST


# ----------------------------------------------------------------------------- scalar problems
def ode_f(s, x):
    """dx/dsigma = x cos(3 sigma) + 0.5 sin(5 sigma): the order tests' problem, x(1) = 1, integrated down to sigma = 0."""
    return x * math.cos(3.0 * s) + 0.5 * math.sin(5.0 * s)


def rk4_reference(f=ode_f, x0=1.0, s0=1.0, s1=0.0, n=20000):
    h, x, s = (s1 - s0) / n, float(x0), float(s0)
    for _ in range(n):
        k1 = f(s, x)
        k2 = f(s + h / 2, x + h / 2 * k1)
        k3 = f(s + h / 2, x + h / 2 * k2)
        k4 = f(s + h, x + h * k3)
        x += h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        s += h
    return x


def table_loop64(sigmas, table, f=ode_f, x0=1.0):
    """x after the rows of `table` ([n, 8] fp32: c_0 in column 0, dt in column 2, flags in column 4, c_1 / c_2 in columns 6 / 7),
    every entry taken as the fp64 number it is, the velocity of row i evaluated at sigmas[i]."""
    x, hist = float(x0), []
    for i in range(table.shape[0]):
        row = [float(t) for t in table[i].double()]
        v = f(float(sigmas[i].double()), x)
        deriv = row[0] * v
        if int(row[4]) & STEP_HIST:
            if row[6] != 0.0:
                deriv += row[6] * hist[-1]
            if row[7] != 0.0:
                deriv += row[7] * hist[-2]
        x += deriv * row[2]
        hist.append(v)
    return x
