// SX-defined models beyond the reference's double pendulum, generated through the same ModelGenerator calls
// (create_model / generate_c_code / compile_model) -- used by the tests to exercise the three kinematic
// structures the kernels handle (sqp_lane.h a_mul):
//   cart_pole       x = [p, th, p_dot, th_dot], u = [F]       second order, nq = 2 (tanh friction, division)
//   unicycle        x = [px, py, th, v],        u = [a, w]    first order,  nq = 0 (sqrt drag)
//   motor_pendulum  x = [th, om, i],            u = [V]       mixed,        nq = 1, na = 2 (exp, sq)
// and one model at the width limit of the 16-lane kernels (nx + nu = 16: one lane per column no longer fits):
//   mass_chain      x = [p0..p5, v0..v5],       u = [f0..f3]  second order, nq = 6: six masses in a row coupled by
//                   sinusoidal springs, forces on masses 0, 2, 3 and 5
// The same equations are restated in sympy in tests/test_sx_models.py.
//   sx_model_zoo <model> <N> [linear]      writes <model>{,_model.h,_linear_functions.{c,so},.so,.json} in the cwd
#include <Mahi/Mpc.hpp>

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace casadi;
using namespace mahi::mpc;

int main(int argc, char* argv[]) {
    if (argc < 3) {
        std::cerr << "usage: sx_model_zoo cart_pole|unicycle|motor_pendulum|mass_chain N [linear]" << std::endl;
        return 2;
    }
    const std::string which = argv[1];
    const int N = std::atoi(argv[2]);
    const bool linear = argc > 3 && !std::strcmp(argv[3], "linear");
    SX x, x_dot, u;
    if (which == "cart_pole") {
        const double mc = 1.0, mp = 0.1, l = 0.5, g = 9.81, fr = 0.2;
        SX p = SX::sym("p"), th = SX::sym("th"), p_dot = SX::sym("p_dot"), th_dot = SX::sym("th_dot");
        SX F = SX::sym("F");
        SX tmp = (F - fr * tanh(5 * p_dot) + mp * l * th_dot * th_dot * sin(th)) / (mc + mp);
        SX th_ddot = (g * sin(th) - cos(th) * tmp) / (l * (4.0 / 3.0 - mp * cos(th) * cos(th) / (mc + mp)));
        SX p_ddot = tmp - mp * l * th_ddot * cos(th) / (mc + mp);
        x = SX::vertcat({p, th, p_dot, th_dot});
        x_dot = SX::vertcat({p_dot, th_dot, p_ddot, th_ddot});
        u = F;
    } else if (which == "unicycle") {
        SX px = SX::sym("px"), py = SX::sym("py"), th = SX::sym("th"), v = SX::sym("v");
        SX a = SX::sym("a"), w = SX::sym("w");
        x = SX::vertcat({px, py, th, v});
        x_dot = SX::vertcat({v * cos(th), v * sin(th), w, a - 0.05 * v * sqrt(1 + v * v)});
        u = SX::vertcat({a, w});
    } else if (which == "motor_pendulum") {
        const double J = 0.01, b = 0.1, K = 0.05, R = 1.0, Lm = 0.5, m = 0.2, g = 9.81, l = 0.3;
        SX th = SX::sym("th"), om = SX::sym("om"), i = SX::sym("i"), V = SX::sym("V");
        SX om_dot = (K * i - b * om - m * g * l * sin(th)) / J;
        SX i_dot = (V - R * (1 + 0.1 * exp(-sq(i))) * i - K * om) / Lm;
        x = SX::vertcat({th, om, i});
        x_dot = SX::vertcat({om, om_dot, i_dot});
        u = V;
    } else if (which == "mass_chain") {
        std::vector<SX> p, v, f, xs, xd;
        for (int i = 0; i < 6; ++i) p.push_back(SX::sym("p" + std::to_string(i)));
        for (int i = 0; i < 6; ++i) v.push_back(SX::sym("v" + std::to_string(i)));
        for (int i = 0; i < 4; ++i) f.push_back(SX::sym("f" + std::to_string(i)));
        const int actuator[6] = {0, -1, 1, 2, -1, 3};
        xs = p;
        xs.insert(xs.end(), v.begin(), v.end());
        xd = v;
        for (int i = 0; i < 6; ++i) {
            SX a = -0.3 * v[i] - 2.0 * sin(p[i]);
            if (i > 0) a = a + 5.0 * sin(p[i - 1] - p[i]);
            if (i < 5) a = a + 5.0 * sin(p[i + 1] - p[i]);
            if (actuator[i] >= 0) a = a + f[actuator[i]];
            xd.push_back(a);
        }
        x = SX::vertcat(xs);
        x_dot = SX::vertcat(xd);
        u = SX::vertcat(f);
    } else {
        std::cerr << "unknown model " << which << std::endl;
        return 2;
    }
    const std::string name = (linear ? "linear_" : "") + which;
    ModelParameters mp(name, x.size1(), u.size1(), mahi::util::milliseconds(10), N, linear);
    ModelGenerator gen(mp, x, x_dot, u);
    gen.create_model();
    gen.generate_c_code();
    gen.compile_model();
    std::cout << name << ": nq = " << gen.kinematic_rows() << std::endl;
    return 0;
}
