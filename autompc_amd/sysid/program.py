"""Analytic simulation dynamics as a straight-line program that runs on the device.

The closed-form dynamics of the reference's MuJoCo-free benchmarks (benchmarks/cartpole.py, cartpole_v2.py) are a
handful of ``+ - * / sin cos`` on the observation and the control.  ``DynamicsProgram.trace(system, fn)`` calls such
a function ONCE with symbolic operands and records what it does as a list of three-address instructions over value
slots; the list is then

* evaluated on the host with numpy, instruction by instruction (``pred`` / ``pred_batch`` / ``__call__``), and
* interpreted on the device, one row per lane (csrc/program_kernels.hpp): ``pred_batch(..., device=True)``,
  ``stage_into(handle)`` -- which makes the program the ``surrogate`` of every closed loop -- and ``rollout``.

Program format: ``code`` [n_instr][4] int32 rows ``(op, dst, a, b)``, ``consts`` [n_const] float64, ``out_slot``
[nx] int32.  Slots ``0 .. nx+nu-1`` hold ``[obs | ctrl]`` on entry; output ``i`` is slot ``out_slot[i]``.

    0 const  v[dst] = consts[a]        1 add  2 sub  3 mul  4 div       v[dst] = v[a] op v[b]
    5 neg  6 sin  7 cos  8 exp  9 sqrt  10 abs  11 tanh                 v[dst] = f(v[a])
    12 powi  v[dst] = v[a] ** b  (b an integer, |b| <= 64)              13 min  14 max

Rounding contract: instructions are recorded in Python's evaluation order -- no re-association, no common
subexpressions merged -- and every instruction rounds once, on the host and on the device alike.  Integer powers are
repeated multiplication left to right (``((x*x)*x)*x``; a negative exponent takes the reciprocal of that) on both
sides, not ``np.power``.  So add / sub / mul / div / sqrt / abs / min / max / powi agree between host and device
bit for bit; sin / cos / exp / tanh agree to the device library's few ulp.

Limits: ``MAX_SLOTS`` = 256 value slots live at once (slots are reused after a value's last use) and ``MAX_INSTR`` =
4096 instructions, at most 64 observations and 16 controls: 256 slots plus the rollout's 64 hand-over rows, for 64
lanes of f64, are the 160 KB of LDS a workgroup can have.  A program beyond them raises ``ValueError``.

Refused while tracing, with ``TypeError``: anything that would make the recorded list depend on the data --
``bool()`` of a symbol, a comparison used in ``if``, ``np.where``, a ufunc outside the table above.  No branch is
ever baked in silently.  A ``DynamicsProgram`` has no Jacobians (``pred_diff*`` raise) and cannot be a controller's
model.

``DifferentiableProgram`` (``prog.differentiable()``, or ``DifferentiableProgram.trace`` / ``from_code``) is the opt-in
subclass that has both.  At construction it derives the JVP program (Jacobian-vector product, forward mode) from the
stored ``code``: a program of the same format with ``2(nx+nu)`` inputs ``[x | u | dx | du]`` and ``2nx`` outputs
``[f | J.(dx, du)]``.  Every write gets a fresh value id, values and tangents are emitted in list order, a tangent
known to be zero (constants, values that depend on no input) is folded away, and ``_allocate`` assigns the slots; the
folded program is the definition.  Tangent rules (``r`` the instruction's own result, ``ta`` / ``tb`` the operands'
tangents, every new instruction in the order written):

    add sub neg   ta + tb, ta - tb, -ta                 mul   (ta * b) + (a * tb)
    div           (ta - r * tb) / b                     sin cos   cos(a) * ta, -(sin(a) * ta)
    exp sqrt tanh r * ta, ta / (r + r), (1 - r * r) * ta          abs   sign(a) * ta
    powi n        0 | ta | (n * powi(a, n-1)) * ta | n < 0: (n * (r / a)) * ta
    min(a, b)     s = lt(b, a): (s * tb) + ((1 - s) * ta)         max(a, b)   s = lt(a, b), the same tangent

Two opcodes exist for derived programs (``from_code`` / ``validate`` accept them, the tracer still refuses comparisons
and ``np.sign``); both are exact, so the rounding contract covers JVP programs unchanged:

    15 sign  v[dst] = sign(v[a])  (-1, 0, +1; NaN stays NaN)       16 lt  v[dst] = v[a] < v[b] ? 1 : 0

A ``DifferentiableProgram`` has ``pred_diff`` / ``pred_diff_batch`` (host: the JVP program once per unit direction;
device: one lane per (row, direction), csrc/program_kernels.hpp), ``stage_into`` stages the program and then its JVP,
and a handle with both is an MPPI controller model (csrc/mppi_program_kernels.hpp).  A JVP beyond ``MAX_SLOTS`` /
``MAX_INSTR`` raises ``ValueError`` at construction.  ``DifferentiableProgram(..., ilqr=True)`` /
``prog.differentiable(ilqr=True)`` / ``trace`` / ``from_code`` with ``ilqr=True`` additionally make it an iLQR
controller model (``stage_into`` sets the handle's flag after the JVP; f64, csrc/ilqr_kernels.hpp DYN = 3).
"""
import heapq
import numbers

import numpy as np

from .. import _lib
from .model import Model

(OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_SIN, OP_COS, OP_EXP, OP_SQRT, OP_ABS, OP_TANH, OP_POWI,
 OP_MIN, OP_MAX, OP_SIGN, OP_LT) = range(17)
OP_NAMES = ("const", "add", "sub", "mul", "div", "neg", "sin", "cos", "exp", "sqrt", "abs", "tanh", "powi", "min",
            "max", "sign", "lt")
_TRACED = OP_NAMES[1:OP_SIGN]          # what the tracer records; sign / lt appear in derived (JVP) programs only
_BINARY = (OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_MIN, OP_MAX, OP_LT)
_UNARY = (OP_NEG, OP_SIN, OP_COS, OP_EXP, OP_SQRT, OP_ABS, OP_TANH, OP_SIGN)
MAX_SLOTS, MAX_INSTR, MAX_POW, MAX_OBS, MAX_CTRL = 256, 4096, 64, 64, 16


def powi(x, n):
    """x ** n for an integer n as the device computes it: ((x * x) * x) * ..., then the reciprocal for n < 0."""
    e = abs(int(n))
    r = np.ones_like(x) if e == 0 else x
    for _ in range(1, e):
        r = r * x
    return (np.ones_like(x) / r) if n < 0 else r


def _lt(a, b):
    return (a < b).astype(a.dtype)


_HOST_UNARY = {OP_NEG: np.negative, OP_SIN: np.sin, OP_COS: np.cos, OP_EXP: np.exp, OP_SQRT: np.sqrt,
               OP_ABS: np.absolute, OP_TANH: np.tanh, OP_SIGN: np.sign}
_HOST_BINARY = {OP_ADD: np.add, OP_SUB: np.subtract, OP_MUL: np.multiply, OP_DIV: np.divide, OP_MIN: np.minimum,
                OP_MAX: np.maximum, OP_LT: _lt}


# ---------------------------------------------------------------------------------------------------------------
# tracing
# ---------------------------------------------------------------------------------------------------------------
class _Tape:
    def __init__(self, n_in):
        self.n_in = n_in
        self.instr = []          # (op, a, b): value ids (inputs 0..n_in-1, instruction k defines n_in + k)
        self.consts = []
        self._const_id = {}      # bit pattern -> (pool index, value id): a constant is loaded once

    def emit(self, op, a, b=0):
        if len(self.instr) >= MAX_INSTR:
            raise ValueError("the traced dynamics need more than %d instructions (DynamicsProgram.MAX_INSTR)"
                             % MAX_INSTR)
        self.instr.append((op, a, b))
        return _Sym(self, self.n_in + len(self.instr) - 1)

    def const(self, value):
        value = float(value)
        key = np.float64(value).tobytes()
        if key not in self._const_id:
            self.consts.append(value)
            self._const_id[key] = self.emit(OP_CONST, len(self.consts) - 1)
        return self._const_id[key]

    def sym(self, x, what):
        if isinstance(x, _Sym):
            if x.tape is not self:
                raise TypeError("a symbol of another trace reached this one")
            return x
        if isinstance(x, _Cond):
            x.__bool__()
        if isinstance(x, (bool, np.bool_)):
            raise TypeError("DynamicsProgram.trace: a boolean operand in %s: comparisons cannot be recorded" % what)
        if isinstance(x, numbers.Real) or (isinstance(x, np.ndarray) and x.ndim == 0 and x.dtype.kind in "fiu"):
            return self.const(x)
        raise TypeError("DynamicsProgram.trace: cannot record %s with an operand of type %s" % (what, type(x).__name__))


class _Cond:
    """What comparing a symbol gives: nothing a straight-line program could branch on."""

    def __bool__(self):
        raise TypeError("DynamicsProgram.trace: the dynamics compare a traced value (if / while / np.where / np.clip "
                        "of a whole vector): the recorded program would depend on the data.  Write the choice with "
                        "np.minimum / np.maximum / np.clip on the elements, or keep these dynamics on the host")

    __array_ufunc__ = None


_UFUNC_OPS = {np.add: OP_ADD, np.subtract: OP_SUB, np.multiply: OP_MUL, np.divide: OP_DIV, np.negative: OP_NEG,
              np.sin: OP_SIN, np.cos: OP_COS, np.exp: OP_EXP, np.sqrt: OP_SQRT, np.absolute: OP_ABS,
              np.fabs: OP_ABS, np.tanh: OP_TANH, np.minimum: OP_MIN, np.maximum: OP_MAX}


class _Sym:
    """One traced value.  Arithmetic on it appends an instruction to its tape and returns the new value."""
    __slots__ = ("tape", "vid")

    def __init__(self, tape, vid):
        self.tape, self.vid = tape, vid

    def _bin(self, op, other, swap=False):
        try:
            o = self.tape.sym(other, OP_NAMES[op])
        except TypeError:
            if isinstance(other, (np.ndarray, list, tuple)):
                return NotImplemented
            raise
        a, b = (o, self) if swap else (self, o)
        return self.tape.emit(op, a.vid, b.vid)

    def _un(self, op):
        return self.tape.emit(op, self.vid)

    def __add__(self, o): return self._bin(OP_ADD, o)
    def __radd__(self, o): return self._bin(OP_ADD, o, True)
    def __sub__(self, o): return self._bin(OP_SUB, o)
    def __rsub__(self, o): return self._bin(OP_SUB, o, True)
    def __mul__(self, o): return self._bin(OP_MUL, o)
    def __rmul__(self, o): return self._bin(OP_MUL, o, True)
    def __truediv__(self, o): return self._bin(OP_DIV, o)
    def __rtruediv__(self, o): return self._bin(OP_DIV, o, True)
    def __neg__(self): return self._un(OP_NEG)
    def __pos__(self): return self
    def __abs__(self): return self._un(OP_ABS)

    def __pow__(self, n, mod=None):
        if mod is not None or isinstance(n, (_Sym, bool)) or not isinstance(n, numbers.Real) or n != int(n) \
                or abs(int(n)) > MAX_POW:
            raise TypeError("DynamicsProgram.trace: only integer powers up to %d of a traced value are recorded "
                            "(got %r); write a square root as np.sqrt" % (MAX_POW, n))
        return self.tape.emit(OP_POWI, self.vid, int(n))

    def __rpow__(self, base):
        raise TypeError("DynamicsProgram.trace: a traced value as an exponent is not recorded; write c ** x as "
                        "np.exp(np.log(c) * x)")

    # what numpy's object loops call on the elements of an object array
    def sin(self): return self._un(OP_SIN)
    def cos(self): return self._un(OP_COS)
    def exp(self): return self._un(OP_EXP)
    def sqrt(self): return self._un(OP_SQRT)
    def tanh(self): return self._un(OP_TANH)

    def clip(self, min=None, max=None, out=None, **kwargs):       # np.clip(x, lo, hi) on one element
        if out is not None or kwargs:
            raise TypeError("DynamicsProgram.trace: np.clip with out= / keywords is not recorded")
        r = self
        if min is not None:
            r = r._bin(OP_MAX, min)
        if max is not None:
            r = r._bin(OP_MIN, max)
        return r

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        if method != "__call__" or kwargs:
            raise TypeError("DynamicsProgram.trace: %s.%s with keywords / reductions is not recorded" % (ufunc.__name__, method))
        if any(isinstance(x, np.ndarray) and x.ndim > 0 for x in inputs):
            # an array operand: as a 0-d object array this value goes through numpy's object loop, which comes
            # back element by element
            boxed = []
            for x in inputs:
                if isinstance(x, _Sym):
                    cell = np.empty((), dtype=object)
                    cell[()] = x
                    x = cell
                boxed.append(x)
            return ufunc(*boxed)
        if ufunc is np.power:
            if inputs[0] is self:
                return self.__pow__(inputs[1].item() if isinstance(inputs[1], np.ndarray) else inputs[1])
            return self.__rpow__(inputs[0])
        if ufunc is np.square:
            return self.__pow__(2)
        if ufunc is np.positive:
            return self
        op = _UFUNC_OPS.get(ufunc)
        if op is None:
            raise TypeError("DynamicsProgram.trace: numpy.%s is not an operation a program records (it knows: %s)"
                            % (ufunc.__name__, ", ".join(_TRACED)))
        if op in _UNARY:
            return self._un(op)
        a, b = (self.tape.sym(x, OP_NAMES[op]) for x in inputs)
        return self.tape.emit(op, a.vid, b.vid)

    def _compare(self, other): return _Cond()
    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _compare
    __hash__ = None

    def __bool__(self):
        return _Cond().__bool__()

    def __float__(self):
        raise TypeError("DynamicsProgram.trace: a traced value was converted to a float (math.sin, float(), a numeric "
                        "array): use numpy's functions on the operands themselves")

    __int__ = __index__ = __float__

    def __repr__(self):
        return "<traced value %d>" % self.vid


def _allocate(n_in, instr, outputs, max_slots=MAX_SLOTS):
    """Value ids -> slots, reusing a slot after its value's last use.  Inputs sit in slots 0..n_in-1 (reusable after
    their last use too: every step reloads them); outputs stay live to the end.  max_slots=None: no limit here, the
    caller looks at the count returned."""
    n_val = n_in + len(instr)
    last = [-1] * n_val
    for k, (op, a, b) in enumerate(instr):
        if op != OP_CONST:
            last[a] = k
            if op in _BINARY:
                last[b] = k
    for v in outputs:
        last[v] = len(instr)
    slot = list(range(n_in)) + [0] * len(instr)
    free, top = [], n_in
    for v in range(n_in):
        if last[v] < 0:
            heapq.heappush(free, v)
    code = np.zeros((len(instr), 4), dtype=np.int32)
    for k, (op, a, b) in enumerate(instr):
        sa = a if op == OP_CONST else slot[a]
        sb = slot[b] if op in _BINARY else b
        if op != OP_CONST:                          # operands that die here free their slots: dst may be one of them
            for v in {a, b} if op in _BINARY else {a}:
                if last[v] == k:
                    heapq.heappush(free, slot[v])
        if free:
            d = heapq.heappop(free)
        else:
            d, top = top, top + 1
            if max_slots is not None and top > max_slots:
                raise ValueError("the traced dynamics keep more than %d values alive at once "
                                 "(DynamicsProgram.MAX_SLOTS: the slots of 64 rows live in LDS)" % MAX_SLOTS)
        v = n_in + k
        slot[v] = d
        code[k] = (op, d, sa, sb)
        if last[v] < 0:                             # a value nobody reads
            heapq.heappush(free, d)
    return code, np.array([slot[v] for v in outputs], dtype=np.int32), top


def validate(nx, nu, n_slots, code, n_const, out_slot, jvp=False):
    """The checks ampc_set_program makes (ValueError here), on the host arrays; jvp: those of ampc_set_program_jvp,
    for a program of 2 (nx + nu) inputs and 2 nx outputs."""
    if not (1 <= nx <= MAX_OBS and 1 <= nu <= MAX_CTRL):
        raise ValueError("a program takes 1..%d observations and 1..%d controls" % (MAX_OBS, MAX_CTRL))
    n_in, n_out = (2 * (nx + nu), 2 * nx) if jvp else (nx + nu, nx)
    if len(out_slot) != n_out:
        raise ValueError("out_slot needs %d entries, not %d" % (n_out, len(out_slot)))
    if not n_in <= n_slots <= MAX_SLOTS:
        raise ValueError("n_slots = %d: must cover the %d inputs and be at most %d" % (n_slots, n_in, MAX_SLOTS))
    if len(code) > MAX_INSTR:
        raise ValueError("%d instructions: at most %d" % (len(code), MAX_INSTR))
    defined = [True] * n_in + [False] * (n_slots - n_in)
    for k, (op, d, a, b) in enumerate(np.asarray(code).tolist()):
        if not 0 <= op < len(OP_NAMES):
            raise ValueError("instruction %d: unknown opcode %d" % (k, op))
        if not 0 <= d < n_slots:
            raise ValueError("instruction %d: destination slot %d outside 0..%d" % (k, d, n_slots - 1))
        if op == OP_CONST:
            if not 0 <= a < n_const:
                raise ValueError("instruction %d: constant index %d outside 0..%d" % (k, a, n_const - 1))
        else:
            for s in (a, b) if op in _BINARY else (a,):
                if not 0 <= s < n_slots:
                    raise ValueError("instruction %d: operand slot %d outside 0..%d" % (k, s, n_slots - 1))
                if not defined[s]:
                    raise ValueError("instruction %d reads slot %d before anything wrote it" % (k, s))
            if op == OP_POWI and abs(b) > MAX_POW:
                raise ValueError("instruction %d: exponent %d outside -%d..%d" % (k, b, MAX_POW, MAX_POW))
        defined[d] = True
    for i, s in enumerate(np.asarray(out_slot).tolist()):
        if not 0 <= s < n_slots or not defined[s]:
            raise ValueError("out_slot[%d] = %d names no defined slot" % (i, s))


def _run(p, V, dtype):
    """The list of `p` (code, consts, out_slot, n_slots) on the columns of V [n][n_in], in order, every instruction
    in `dtype`: [n][len(out_slot)]."""
    consts = p.consts.astype(dtype)
    v = [None] * p.n_slots
    for i in range(V.shape[1]):
        v[i] = V[:, i].copy()
    with np.errstate(all="ignore"):
        for op, d, a, b in p.code.tolist():
            if op == OP_CONST:
                v[d] = np.full(V.shape[0], consts[a], dtype=dtype)
            elif op == OP_POWI:
                v[d] = powi(v[a], b)
            elif op in _HOST_BINARY:
                v[d] = _HOST_BINARY[op](v[a], v[b])
            else:
                v[d] = _HOST_UNARY[op](v[a])
    return np.stack([v[s] for s in p.out_slot.tolist()], axis=1)


class DynamicsProgram(Model):
    """x' = f(x, u) as a recorded straight-line program: a simulation model whose state is the observation."""
    MAX_SLOTS, MAX_INSTR = MAX_SLOTS, MAX_INSTR

    def __init__(self, system, code, consts, out_slot, n_slots, device=0):
        super().__init__(system)
        self.code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 4)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
        self.out_slot = np.ascontiguousarray(out_slot, dtype=np.int32).reshape(-1)
        self.n_slots = int(n_slots)
        self.device = device
        if self.out_slot.shape[0] != system.obs_dim:
            raise ValueError("out_slot needs one entry per observation (%d)" % system.obs_dim)
        validate(system.obs_dim, system.ctrl_dim, self.n_slots, self.code, self.consts.shape[0], self.out_slot)
        self._handles = {}

    # -- construction -------------------------------------------------------------------------------------------
    @classmethod
    def from_code(cls, system, code, consts, out_slot, n_slots=None, device=0, **kw):
        """From the raw arrays (module docstring); n_slots defaults to the highest slot named + 1.  Further keywords
        go to the class (DifferentiableProgram: ilqr=)."""
        code = np.asarray(code, dtype=np.int32).reshape(-1, 4)
        if n_slots is None:
            named = [system.obs_dim + system.ctrl_dim - 1] + [int(s) for s in np.asarray(out_slot).reshape(-1)]
            for op, d, a, b in code.tolist():
                named += [d] + ([a] if op != OP_CONST else []) + ([b] if op in _BINARY else [])
            n_slots = max(named) + 1
        return cls(system, code, consts, out_slot, n_slots, device=device, **kw)

    @classmethod
    def trace(cls, system, fn, device=0, **kw):
        """Record ``fn(obs, ctrl)``: called once, with object arrays of traced values of the system's dimensions.
        Further keywords go to the class (DifferentiableProgram: ilqr=)."""
        nx, nu = system.obs_dim, system.ctrl_dim
        tape = _Tape(nx + nu)
        obs = np.empty(nx, dtype=object)
        ctrl = np.empty(nu, dtype=object)
        for i in range(nx):
            obs[i] = _Sym(tape, i)
        for j in range(nu):
            ctrl[j] = _Sym(tape, nx + j)
        res = fn(obs, ctrl)
        if isinstance(res, (_Sym, numbers.Real)):
            res = [res]
        res = list(res)
        if len(res) != nx:
            raise ValueError("the dynamics returned %d values for %d observations" % (len(res), nx))
        outputs = [tape.sym(r, "the result").vid for r in res]
        code, out_slot, n_slots = _allocate(nx + nu, tape.instr, outputs)
        return cls(system, code, tape.consts, out_slot, max(n_slots, nx + nu), device=device, **kw)

    # -- Model surface --------------------------------------------------------------------------------------------
    @property
    def state_dim(self):
        return self.system.obs_dim

    def traj_to_state(self, traj):
        return traj[-1].obs.copy()

    def update_state(self, state, new_ctrl, new_obs):
        return np.array(new_obs, dtype=np.float64)

    def evaluate(self, states, ctrls, dtype=np.float64):
        """The recorded list on the host, in order, every instruction in `dtype` (float64, or float32 as an f32
        handle computes: the constants are rounded to it first)."""
        nx, nu = self.system.obs_dim, self.system.ctrl_dim
        X = np.asarray(states, dtype=dtype).reshape(-1, nx)
        U = np.asarray(ctrls, dtype=dtype).reshape(-1, nu)
        if X.shape[0] != U.shape[0]:
            raise ValueError("states and ctrls need the same number of rows")
        return _run(self, np.concatenate([X, U], axis=1), dtype)

    def pred(self, state, ctrl):
        return self.evaluate(np.asarray(state, dtype=np.float64)[None, :], np.atleast_1d(ctrl)[None, :])[0]

    def __call__(self, obs, ctrl):
        """``dynamics(y, u)`` of the generators and of ``simulate(dynamics=...)``: a fresh array, `obs` untouched."""
        return self.pred(obs, ctrl)

    def pred_batch(self, states, ctrls, device=False, precision="f64"):
        if device:
            return self._dev(precision).pred_batch(states, ctrls)
        return self.evaluate(states, ctrls)

    def rollout(self, x0, ctrls, device=False, precision="f64"):
        """obs [n][T+1][nx] of n trajectories from x0 [n][nx] under ctrls [n][T][nu]: one launch on the device
        (ampc_program_rollout), or the same steps on the host."""
        x0 = np.asarray(x0, dtype=np.float64)
        ctrls = np.asarray(ctrls, dtype=np.float64)
        n, T = x0.shape[0], ctrls.shape[1]
        if device:
            return self._dev(precision).program_rollout(x0, ctrls)
        obs = np.empty((n, T + 1, self.system.obs_dim))
        obs[:, 0] = x0
        for t in range(T):
            obs[:, t + 1] = self.evaluate(obs[:, t], ctrls[:, t])
        return obs

    # -- device -----------------------------------------------------------------------------------------------------
    def stage_into(self, handle):
        handle.set_program(self.system.obs_dim, self.system.ctrl_dim, self.n_slots, self.code, self.consts,
                           self.out_slot)

    def _dev(self, precision="f64"):
        if precision not in self._handles:
            h = _lib.Handle(self.device, precision)
            self.stage_into(h)
            self._handles[precision] = h
        return self._handles[precision]

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_handles"] = {}
        return state

    def differentiable(self, ilqr=False):
        """The same arrays as a DifferentiableProgram: Jacobians, and an MPPI controller model; ilqr=True: an iLQR
        controller model as well (DifferentiableProgram.ilqr_plans)."""
        return DifferentiableProgram(self.system, self.code, self.consts, self.out_slot, self.n_slots,
                                     device=self.device, ilqr=ilqr)


# ---------------------------------------------------------------------------------------------------------------
# forward-mode derivative of a program, in the same instruction set
# ---------------------------------------------------------------------------------------------------------------
class ProgramArrays:
    """The arrays of a program: code, consts, out_slot, n_slots (module docstring), for n_in input slots."""

    def __init__(self, n_in, code, consts, out_slot, n_slots):
        self.n_in = int(n_in)
        self.code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 4)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
        self.out_slot = np.ascontiguousarray(out_slot, dtype=np.int32).reshape(-1)
        self.n_slots = int(n_slots)

    def evaluate(self, inputs, dtype=np.float64):
        """out [n][len(out_slot)] for inputs [n][n_in], every instruction in `dtype`."""
        return _run(self, np.asarray(inputs, dtype=dtype).reshape(-1, self.n_in), dtype)


def derive_jvp(nx, nu, code, consts, out_slot):
    """The JVP program of (code, consts, out_slot) as ProgramArrays with 2 (nx + nu) inputs [x | u | dx | du] and
    2 nx outputs [f | J . (dx, du)] (module docstring).  No limit is checked here: n_slots and the instruction count
    are whatever the derivative needs."""
    nv = nx + nu
    n_in = 2 * nv
    instr, pool, const_id = [], [float(c) for c in np.asarray(consts, dtype=np.float64)], {}

    def emit(op, a, b=0):
        instr.append((op, a, b))
        return n_in + len(instr) - 1

    def const(value):                    # a constant the rules need (1, n, 0): loaded once, at its first use
        key = np.float64(value).tobytes()
        if key not in const_id:
            pool.append(float(value))
            const_id[key] = emit(OP_CONST, len(pool) - 1)
        return const_id[key]

    cur = list(range(nv)) + [None] * MAX_SLOTS         # slot -> the value id it holds now
    tan = {i: nv + i for i in range(nv)}               # value id -> its tangent's value id; absent: zero

    def select(s, ta, tb):               # (s * tb) + ((1 - s) * ta)
        m1 = emit(OP_MUL, s, tb) if tb is not None else None
        m2 = emit(OP_MUL, emit(OP_SUB, const(1.0), s), ta) if ta is not None else None
        if m1 is None or m2 is None:
            return m1 if m2 is None else m2
        return emit(OP_ADD, m1, m2)

    for op, d, a, b in np.asarray(code, dtype=np.int64).reshape(-1, 4).tolist():
        if op == OP_CONST:
            cur[d] = emit(OP_CONST, a)
            continue
        va, vb = cur[a], (cur[b] if op in _BINARY else b)
        ta, tb = tan.get(va), (tan.get(vb) if op in _BINARY else None)
        r = emit(op, va, vb)
        t = None
        if op == OP_ADD:
            t = emit(OP_ADD, ta, tb) if ta is not None and tb is not None else (ta if tb is None else tb)
        elif op == OP_SUB:
            if tb is None:
                t = ta
            else:
                t = emit(OP_SUB, ta, tb) if ta is not None else emit(OP_NEG, tb)
        elif op == OP_NEG:
            t = emit(OP_NEG, ta) if ta is not None else None
        elif op == OP_MUL:
            m1 = emit(OP_MUL, ta, vb) if ta is not None else None
            m2 = emit(OP_MUL, va, tb) if tb is not None else None
            t = emit(OP_ADD, m1, m2) if m1 is not None and m2 is not None else (m1 if m2 is None else m2)
        elif op == OP_DIV:
            if tb is None:
                t = emit(OP_DIV, ta, vb) if ta is not None else None
            else:
                m = emit(OP_MUL, r, tb)
                t = emit(OP_DIV, emit(OP_SUB, ta, m) if ta is not None else emit(OP_NEG, m), vb)
        elif op == OP_MIN:
            if ta is not None or tb is not None:
                t = select(emit(OP_LT, vb, va), ta, tb)
        elif op == OP_MAX:
            if ta is not None or tb is not None:
                t = select(emit(OP_LT, va, vb), ta, tb)
        elif ta is None:
            pass                                       # a unary operation, a power or a comparison of a constant
        elif op == OP_SIN:
            t = emit(OP_MUL, emit(OP_COS, va), ta)
        elif op == OP_COS:
            t = emit(OP_NEG, emit(OP_MUL, emit(OP_SIN, va), ta))
        elif op == OP_EXP:
            t = emit(OP_MUL, r, ta)
        elif op == OP_SQRT:
            t = emit(OP_DIV, ta, emit(OP_ADD, r, r))
        elif op == OP_TANH:
            one = const(1.0)
            t = emit(OP_MUL, emit(OP_SUB, one, emit(OP_MUL, r, r)), ta)
        elif op == OP_ABS:
            t = emit(OP_MUL, emit(OP_SIGN, va), ta)
        elif op == OP_POWI:
            n = int(b)
            if n == 1:
                t = ta
            elif n >= 2:
                t = emit(OP_MUL, emit(OP_MUL, const(n), emit(OP_POWI, va, n - 1)), ta)
            elif n < 0:
                t = emit(OP_MUL, emit(OP_MUL, const(n), emit(OP_DIV, r, va)), ta)
        # (sign, lt: piecewise constant -- zero tangent)
        cur[d] = r
        if t is not None:
            tan[r] = t
    outs = [cur[s] for s in np.asarray(out_slot).reshape(-1).tolist()]
    touts = [tan[v] if v in tan else const(0.0) for v in outs]
    jcode, jout, n_slots = _allocate(n_in, instr, outs + touts, max_slots=None)
    return ProgramArrays(n_in, jcode, pool, jout, max(n_slots, n_in))


class DifferentiableProgram(DynamicsProgram):
    """A DynamicsProgram with exact Jacobians: its JVP program (`jvp`: code, consts, out_slot, n_slots) is derived at
    construction and staged beside the program, which also makes the handle an MPPI controller model.

    ilqr=True (attribute ``ilqr_plans``) is the opt-in for iLQR plans: ``stage_into`` then calls
    ``handle.set_program_ilqr()`` after the JVP, and ``IterativeLQR(system, task, prog, H)``,
    ``IlqrCandidateEvaluator(system, task, prog, surrogate=...)`` and a tuner's ``truedyn_evaluator`` take the program as
    their controller model: the perfect-model iLQR controller (f64).  Without it they are refused in the library, as a
    plain program is."""

    def __init__(self, system, code, consts, out_slot, n_slots, device=0, ilqr=False):
        super().__init__(system, code, consts, out_slot, n_slots, device=device)
        self.ilqr_plans = bool(ilqr)
        nx, nu = system.obs_dim, system.ctrl_dim
        self.jvp = derive_jvp(nx, nu, self.code, self.consts, self.out_slot)
        if self.jvp.n_slots > MAX_SLOTS or self.jvp.code.shape[0] > MAX_INSTR:
            raise ValueError("the JVP program of these dynamics needs %d value slots and %d instructions "
                             "(the program itself: %d and %d); at most %d slots (DynamicsProgram.MAX_SLOTS) and %d "
                             "instructions (MAX_INSTR)" % (self.jvp.n_slots, self.jvp.code.shape[0], self.n_slots,
                                                           self.code.shape[0], MAX_SLOTS, MAX_INSTR))
        validate(nx, nu, self.jvp.n_slots, self.jvp.code, self.jvp.consts.shape[0], self.jvp.out_slot, jvp=True)

    def differentiable(self, ilqr=False):
        """This program; with ilqr=True and the flag not set yet, a copy of it that has it."""
        if ilqr and not self.ilqr_plans:
            return DifferentiableProgram(self.system, self.code, self.consts, self.out_slot, self.n_slots,
                                         device=self.device, ilqr=True)
        return self

    def evaluate_jvp(self, states, ctrls, dtype=np.float64):
        """(next [n][nx], jx [n][nx][nx], ju [n][nx][nu]) from the JVP program on the host, once per unit direction,
        every instruction in `dtype` -- what the device computes, lane by lane."""
        nx, nu = self.system.obs_dim, self.system.ctrl_dim
        nv = nx + nu
        X = np.asarray(states, dtype=dtype).reshape(-1, nx)
        U = np.asarray(ctrls, dtype=dtype).reshape(-1, nu)
        if X.shape[0] != U.shape[0]:
            raise ValueError("states and ctrls need the same number of rows")
        n = X.shape[0]
        V = np.zeros((n, nv, 2 * nv), dtype=dtype)
        V[:, :, :nx], V[:, :, nx:nv] = X[:, None, :], U[:, None, :]
        V[:, np.arange(nv), nv + np.arange(nv)] = 1.0
        out = self.jvp.evaluate(V.reshape(n * nv, 2 * nv), dtype).reshape(n, nv, 2 * nx)
        jac = np.ascontiguousarray(out[:, :, nx:].transpose(0, 2, 1))          # [n][i][direction]
        return out[:, 0, :nx].copy(), np.ascontiguousarray(jac[:, :, :nx]), np.ascontiguousarray(jac[:, :, nx:])

    def pred_diff(self, state, ctrl):
        nxt, jx, ju = self.pred_diff_batch(np.asarray(state, dtype=np.float64)[None, :], np.atleast_1d(ctrl)[None, :])
        return nxt[0], jx[0], ju[0]

    def pred_diff_batch(self, states, ctrls, device=False, precision="f64"):
        if device:
            nx, nu = self.system.obs_dim, self.system.ctrl_dim
            return self._dev(precision).pred_diff_batch(np.asarray(states, dtype=np.float64).reshape(-1, nx),
                                                        np.asarray(ctrls, dtype=np.float64).reshape(-1, nu))
        return self.evaluate_jvp(states, ctrls)

    def stage_into(self, handle):
        super().stage_into(handle)
        handle.set_program_jvp(self.jvp.n_slots, self.jvp.code, self.jvp.consts, self.jvp.out_slot)
        if getattr(self, "ilqr_plans", False):
            handle.set_program_ilqr(True)
