"""Energy operators on the sampling path (src/operators/energy_operators.py):
GaussianEnergy (:478-583), PoissonianEnergy (:586-625), InverseGammaEnergy,
StudentTEnergy and BernoulliEnergy (:628-761), StandardHamiltonian
(:764-831), the likelihood chain (:152-200) and the quadratic forms."""
from functools import reduce
from operator import add

import numpy as np

from .. import utilities
from ..domain_tuple import DomainTuple
from ..field import Field
from ..linearization import Linearization
from ..multi_domain import MultiDomain
from ..multi_field import MultiField
from ..sugar import domain_union, makeDomain
from .adder import Adder
from .linear_operator import LinearOperator
from .operator import Operator, _OpChain
from .sampling_enabler import SamplingEnabler
from .sandwich_operator import SandwichOperator
from .scaling_operator import ScalingOperator
from .simple_linear_operators import VdotOperator


class EnergyOperator(Operator):
    _target = DomainTuple.scalar_domain()


class LikelihoodEnergyOperator(EnergyOperator):
    def __init__(self, data_residual, sqrt_data_metric_at):
        self._res = data_residual
        self._sqrt_data_metric_at = sqrt_data_metric_at
        self._name = None

    def normalized_residual(self, x):
        return (self._sqrt_data_metric_at(x) @ self._res).force(x)

    @property
    def data_domain(self):
        return None if self._res is None else self._res.target

    def get_transformation(self):
        raise NotImplementedError

    def __matmul__(self, other):
        return _LikelihoodChain(self, other)

    def __rmatmul__(self, other):
        return _LikelihoodChain(other, self)

    def __add__(self, other):
        if not isinstance(other, LikelihoodEnergyOperator):
            return super().__add__(other)
        return _LikelihoodSum.make([self, other])

    def __radd__(self, other):
        if not isinstance(other, LikelihoodEnergyOperator):
            return NotImplemented
        return _LikelihoodSum.make([other, self])

    def get_metric_at(self, x):
        dtp, f = self.get_transformation()
        bun = f(Linearization.make_var(x)).jac
        return SandwichOperator.make(bun, sampling_dtype=dtp)

    @property
    def name(self):
        return self._name

    @name.setter
    def name(self, x):
        if isinstance(self, _LikelihoodSum):
            raise RuntimeError("a joint likelihood has no name of its own: name its components")
        self._name = x


class _LikelihoodChain(LikelihoodEnergyOperator):
    def __init__(self, op1, op2):
        from .simple_linear_operators import PartialExtractor
        self._op = _OpChain.make((op1, op2))
        self._domain = self._op.domain
        if isinstance(op1, ScalingOperator):
            res = op2._res
            sqrt_data_metric_at = op2._sqrt_data_metric_at
        elif op1._res is None:
            res = None
            sqrt_data_metric_at = None
        else:
            if isinstance(op2.target, MultiDomain):
                extract = PartialExtractor(op2.target, op1._res.domain)
            else:
                extract = Operator.identity_operator(op2.target)
            res = op1._res @ extract @ op2
            sqrt_data_metric_at = lambda x: op1._sqrt_data_metric_at(op2.force(x))  # noqa: E731
        super().__init__(res, sqrt_data_metric_at)
        self.name = (op2 if isinstance(op1, ScalingOperator) else op1).name

    def get_transformation(self):
        scaled_lh = isinstance(self._op._ops[0], ScalingOperator)
        ii = 1 if scaled_lh else 0
        tr = self._op._ops[ii].get_transformation()
        if tr is None:
            return tr
        dtype, trafo = tr
        if scaled_lh:
            trafo = trafo.scale(np.sqrt(self._op._ops[0]._factor))
        return dtype, _OpChain.make((trafo,) + self._op._ops[ii + 1:])

    def apply(self, x):
        self._check_input(x)
        return self._op(x)


class _LikelihoodSum(LikelihoodEnergyOperator):
    """lh1 + lh2 + ...: the joint likelihood of independent data sets
    (energy_operators.py:208-301).  Every component keeps its own slice of the
    transformation's target and of the data residuals, keyed by its name
    (default "Likelihood i"; components with a MultiDomain there contribute
    their keys prefixed by "name: ")."""

    def __init__(self, ops, _callingfrommake=False):
        from .simple_linear_operators import PrependKey
        if not _callingfrommake:
            raise NotImplementedError
        if len({isinstance(op.domain, DomainTuple) for op in ops}) != 1:
            raise RuntimeError("joint likelihood: the components mix DomainTuple and MultiDomain domains")
        self._ops = tuple(ops)
        names = self._all_names()
        if len(set(names)) != len(names):
            raise ValueError(f"joint likelihood: component names collide: {names}")
        relabel, residuals, with_data = [], [], []
        for name, op in zip(names, self._ops):
            if op._res is None:
                continue
            rl = self._relabel(op.data_domain, name, PrependKey)
            relabel.append(rl)
            residuals.append(rl @ op._res)
            with_data.append(op)

        def sqrt_data_metric_at(x):
            return reduce(add, (rl @ op._sqrt_data_metric_at(x) @ rl.adjoint
                                for rl, op in zip(relabel, with_data)))

        res = reduce(add, residuals) if residuals else None
        super().__init__(res, sqrt_data_metric_at if residuals else None)
        self._domain = domain_union([op.domain for op in self._ops])

    @staticmethod
    def _relabel(dom, name, PrependKey):
        """linear map of a component's slice `dom` onto its keys of the joint space"""
        from .simple_linear_operators import ducktape
        if isinstance(dom, MultiDomain):
            return PrependKey(dom, name + ": ")
        return ducktape(None, dom, name)

    @classmethod
    def unpack(cls, ops, res):
        for op in ops:
            if isinstance(op, cls):
                res = cls.unpack(op._ops, res)
            else:
                res = res + [op]
        return res

    @classmethod
    def make(cls, ops):
        flat = cls.unpack(ops, [])
        if any(not isinstance(op, LikelihoodEnergyOperator) for op in flat):
            raise TypeError("joint likelihood: every component must be a LikelihoodEnergyOperator")
        if len(flat) == 1:
            return flat[0]
        return cls(flat, _callingfrommake=True)

    def apply(self, x):
        self._check_input(x)
        if x.jac is None:
            return reduce(add, (op.force(x) for op in self._ops))
        lin = [op(Linearization.make_var(x.val.extract(op.domain), x.want_metric)) for op in self._ops]
        jac = reduce(lambda a, b: a._myadd(b, False), (ll.jac for ll in lin))
        res = x.new(reduce(add, (ll.val for ll in lin)), jac)
        metrics = [ll.metric for ll in lin]
        if all(mm is not None for mm in metrics):
            res = res.add_metric(reduce(add, metrics))
        return res

    def get_transformation(self):
        from .simple_linear_operators import PrependKey
        trs = [op.get_transformation() for op in self._ops]
        if any(tr is None for tr in trs):
            return None
        dtype, parts = {}, []
        for name, (dtp, tr) in zip(self._all_names(), trs):
            if isinstance(tr.target, MultiDomain):
                pre = name + ": "
                for k in tr.target.keys():
                    dtype[pre + k] = dtp[k] if isinstance(dtp, dict) else dtp
                parts.append(PrependKey(tr.target, pre) @ tr)
            else:
                dtype[name] = dtp
                parts.append(tr.ducktape_left(name))
        return dtype, reduce(add, parts)

    def _get_name(self, i):
        name = self._ops[i].name
        return f"Likelihood {i}" if name is None else name

    def _all_names(self):
        return [self._get_name(i) for i in range(len(self._ops))]

    def _simplify_for_constant_input_nontrivial(self, c_inp):
        # the constants are inserted once in front of the whole sum, so the
        # components still see one shared point (and share its model evaluation)
        from .simplify_for_const import InsertionOperator
        return None, self @ InsertionOperator(self.domain, c_inp)

    def __repr__(self):
        subs = []
        for name, op in zip(self._all_names(), self._ops):
            subs += [f"*{name}*", repr(op)]
        return "_LikelihoodSum:\n" + utilities.indent("\n".join(subs))


class Squared2NormOperator(EnergyOperator):
    def __init__(self, domain):
        self._domain = domain

    def apply(self, x):
        self._check_input(x)
        if x.jac is None:
            return x.vdot(x)
        res = x.val.vdot(x.val)
        return x.new(res, VdotOperator(2 * x.val))


class QuadraticFormOperator(EnergyOperator):
    def __init__(self, endo):
        from .endomorphic_operator import EndomorphicOperator
        if not isinstance(endo, EndomorphicOperator):
            raise TypeError("op must be an EndomorphicOperator")
        self._op = endo
        self._domain = endo.domain

    def apply(self, x):
        self._check_input(x)
        if x.jac is None:
            return 0.5 * x.vdot(self._op(x))
        res = 0.5 * x.val.vdot(self._op(x.val))
        return x.new(res, VdotOperator(self._op(x.val)))


def _field_dtype(f):
    from ..utilities import numpy_dtype
    if isinstance(f, Field):
        return numpy_dtype(f.dtype)
    return {k: numpy_dtype(v.dtype) for k, v in f.items()}


class GaussianEnergy(LikelihoodEnergyOperator):
    """0.5 (f-d)^dagger D^-1 (f-d)."""

    def __init__(self, data=None, inverse_covariance=None, domain=None, sampling_dtype=None):
        if inverse_covariance is not None and not isinstance(inverse_covariance, LinearOperator):
            raise TypeError
        self._domain = self._parseDomain(data, inverse_covariance, domain)
        if not isinstance(data, (Field, MultiField)) and data is not None:
            raise TypeError
        self._icov = inverse_covariance
        if inverse_covariance is None:
            self._op = Squared2NormOperator(self._domain).scale(0.5)
            dt = sampling_dtype if data is None else _field_dtype(data)
            self._icov = ScalingOperator(self._domain, 1., dt)
        else:
            self._op = QuadraticFormOperator(inverse_covariance)
            self._icov = inverse_covariance
        self._data = data
        res = Operator.identity_operator(self._domain) if data is None else Adder(data, neg=True)
        super().__init__(res, lambda x: self.get_metric_at(x).get_sqrt())

    @staticmethod
    def _checkEquivalence(olddom, newdom):
        newdom = makeDomain(newdom)
        if olddom is None:
            return newdom
        utilities.check_object_identity(olddom, newdom)
        return newdom

    def _parseDomain(self, data, inverse_covariance, domain):
        dom = None
        if inverse_covariance is not None:
            dom = self._checkEquivalence(dom, inverse_covariance.domain)
        if data is not None:
            dom = self._checkEquivalence(dom, data.domain)
        if domain is not None:
            dom = self._checkEquivalence(dom, domain)
        if dom is None:
            raise ValueError("no domain given")
        return dom

    def apply(self, x):
        self._check_input(x)
        residual = x if self._data is None else x - self._data
        res = self._op(residual).real
        if x.want_metric:
            return res.add_metric(self.get_metric_at(x.val))
        return res

    def get_transformation(self):
        return self._icov.sampling_dtype, self._icov.get_sqrt()

    def __repr__(self):
        return "GaussianEnergy"


class PoissonianEnergy(LikelihoodEnergyOperator):
    """sum(f) - d^T log(f) for integer counts d."""

    def __init__(self, d):
        if not isinstance(d, Field) or d.dtype not in (np.int64, np.int32, __import__("torch").int64,
                                                        __import__("torch").int32):
            raise TypeError("data is of invalid data-type; counts need to be integers")
        if bool((d.val < 0).any().item()):
            raise ValueError("count data is negative and thus can not be Poissonian")
        self._d = d
        self._dfloat = Field(d.domain, d.val.to(__import__("torch").float64))
        self._domain = DomainTuple.make(d.domain)
        super().__init__(Adder(self._dfloat, neg=True), lambda x: self.get_metric_at(x).get_sqrt())

    def apply(self, x):
        self._check_input(x)
        res = x.sum() - x.log().vdot(self._dfloat)
        if not x.want_metric:
            return res
        return res.add_metric(self.get_metric_at(x.val))

    def get_transformation(self):
        return np.float64, 2. * Operator.identity_operator(self._domain).sqrt()


def _flat64(field, cache, key):
    """the values of a real Field as a flat fp64 vector (parameter array of
    nft_lh_eval_batched), made once"""
    if key not in cache:
        cache[key] = field.val.reshape(-1).to(__import__("torch").float64).contiguous()
    return cache[key]


class InverseGammaEnergy(LikelihoodEnergyOperator):
    """sum (alpha + 1) log(f) + beta / f (energy_operators.py:628-680)."""

    def __init__(self, beta, alpha=-0.5):
        from ..sugar import makeOp
        from .simplify_for_const import ConstantOperator
        if not isinstance(beta, Field):
            raise TypeError("beta must be a Field")
        self._domain = DomainTuple.make(beta.domain)
        self._beta = beta
        if np.isscalar(alpha):
            alpha = Field(beta.domain, np.full(beta.shape, alpha))
        elif not isinstance(alpha, Field):
            raise TypeError("alpha must be a scalar or a Field")
        self._alphap1 = alpha + 1
        if utilities.numpy_dtype(beta.dtype) != np.float64:
            raise TypeError("beta must be float64")
        self._sampling_dtype = _field_dtype(beta)
        self._kargs = {}
        super().__init__(2 * ConstantOperator(self._beta, domain=self._domain),
                         lambda x: makeOp(x.reciprocal().sqrt()))

    def apply(self, x):
        self._check_input(x)
        res = x.log().vdot(self._alphap1) + x.reciprocal().vdot(self._beta)
        if not x.want_metric:
            return res
        return res.add_metric(self.get_metric_at(x.val))

    def get_transformation(self):
        from ..sugar import makeOp
        return self._sampling_dtype, makeOp(self._alphap1.sqrt()) @ Operator.identity_operator(self._domain).log()

    def _lh_kernel_args(self):
        """(kind, p0, p1, c0) of nft_lh_eval_batched"""
        from .. import _native
        return (_native.LH_INVGAMMA, _flat64(self._alphap1, self._kargs, "a"),
                _flat64(self._beta, self._kargs, "b"), 0.0)


class StudentTEnergy(LikelihoodEnergyOperator):
    """sum (theta + 1) / 2 log1p(f^2 / theta) (energy_operators.py:683-720);
    theta a scalar or a Field."""

    def __init__(self, domain, theta):
        self._domain = DomainTuple.make(domain)
        self._theta = theta
        self._kargs = {}
        super().__init__(Operator.identity_operator(self._domain), lambda x: self.get_metric_at(x).get_sqrt())

    def apply(self, x):
        self._check_input(x)
        res = (((self._theta + 1) / 2) * (x ** 2 / self._theta).log1p()).sum()
        if not x.want_metric:
            return res
        return res.add_metric(self.get_metric_at(x.val))

    def get_transformation(self):
        from ..sugar import full, makeOp
        th = self._theta
        if not isinstance(th, (Field, MultiField)):
            th = full(self._domain, th)
        return np.float64, makeOp(((th + 1) / (th + 3)).sqrt())

    def _lh_kernel_args(self):
        from .. import _native
        if isinstance(self._theta, Field):
            return _native.LH_STUDENT_T, _flat64(self._theta, self._kargs, "t"), None, 0.0
        return _native.LH_STUDENT_T, None, None, float(self._theta)


class _BernoulliTransform(Operator):
    """t(f) = -2 arctan(sqrt((1 - f) / f)): the map whose Jacobian squares to
    Bernoulli's Fisher metric 1 / (f (1 - f)).  The reference builds it from an
    operator product (energy_operators.py:757-761); here it is ONE pointwise
    operator whose value and derivative come from one native pass
    (nft_lh_transform_pair), so it stays a chain link that the sandwich
    fusion and the batched geoVI pipeline understand."""

    def __init__(self, domain):
        self._domain = self._target = DomainTuple.make(domain)

    @staticmethod
    def pair(f):
        """(t, dt/df) tensors at the tensor f"""
        import torch
        from .. import _native
        if f.dtype not in (torch.float64, torch.float32):
            f = f.to(torch.float64)
        f = f.contiguous()
        return _native.lh_transform_pair(_native.LH_BERNOULLI, f, torch.empty_like(f), torch.empty_like(f))

    def apply(self, x):
        from ..sugar import makeOp
        self._check_input(x)
        lin = x.jac is not None
        t, dt = self.pair((x.val if lin else x).val)
        if not lin:
            return Field(self._domain, t)
        return x.new(Field(self._domain, t), makeOp(Field(self._domain, dt))(x.jac))

    def __repr__(self):
        return "_BernoulliTransform"


class BernoulliEnergy(LikelihoodEnergyOperator):
    """-d^T log(f) - (1 - d)^T log(1 - f) for events d in {0, 1}
    (energy_operators.py:723-761)."""

    def __init__(self, d):
        if not isinstance(d, Field) or not np.issubdtype(utilities.numpy_dtype(d.dtype), np.integer):
            raise TypeError("data must be a Field of integers")
        if bool(((d.val != 0) & (d.val != 1)).any().item()):
            raise ValueError("data must hold only 0 (no event) and 1 (event)")
        self._d = d
        self._dfloat = Field(d.domain, d.val.to(__import__("torch").float64))
        self._domain = DomainTuple.make(d.domain)
        self._kargs = {}
        super().__init__(Adder(self._dfloat, neg=True), lambda x: self.get_metric_at(x).get_sqrt())

    def apply(self, x):
        self._check_input(x)
        res = -x.log().vdot(self._dfloat) + (1. - x).log().vdot(self._dfloat - 1.)
        if not x.want_metric:
            return res
        return res.add_metric(self.get_metric_at(x.val))

    def get_transformation(self):
        return np.float64, _BernoulliTransform(self._domain)

    def _lh_kernel_args(self):
        from .. import _native
        return _native.LH_BERNOULLI, _flat64(self._dfloat, self._kargs, "d"), None, 0.0


class StandardHamiltonian(EnergyOperator):
    """0.5 xi^dagger xi + E_lh(xi) (energy_operators.py:764-831)."""

    def __init__(self, lh, ic_samp=None):
        self._lh = lh
        self._prior = GaussianEnergy(data=None, domain=lh.domain, sampling_dtype=float)
        self._ic_samp = ic_samp
        self._domain = lh.domain

    def apply(self, x):
        self._check_input(x)
        lhx, prx = self._lh(x), self._prior(x)
        if not x.want_metric or self._ic_samp is None:
            return lhx + prx
        met = SamplingEnabler(lhx.metric, prx.metric, self._ic_samp)
        return (lhx + prx).add_metric(met)

    @property
    def prior_energy(self):
        return self._prior

    @property
    def likelihood_energy(self):
        return self._lh

    @property
    def iteration_controller(self):
        return self._ic_samp

    def __repr__(self):
        return "StandardHamiltonian:\n" + utilities.indent(repr(self._lh))

    def _simplify_for_constant_input_nontrivial(self, c_inp):
        # energy_operators.py:829-831: the prior of the constant keys is a
        # constant and drops out; the likelihood gets the constants inserted
        out, lh1 = self._lh.simplify_for_constant_input(c_inp)
        return out, StandardHamiltonian(lh1, self._ic_samp)
