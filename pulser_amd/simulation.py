"""``QutipEmulator``-compatible front-end of the MI355X emulation backend.

Same constructor / ``from_sequence`` / ``run`` / setters / properties, same
exceptions and warnings as ``pulser_simulation.simulation.QutipEmulator``
(pulser-simulation/pulser_simulation/simulation.py:84-1051), with the solver
call (``qutip.sesolve/mesolve``, :729-735) replaced by the HIP engine.  The
RNG call order on the global ``np.random`` stream is preserved: noise
trajectories at construction (:208), the hidden noiseless ``HamiltonianData``
behind ``set_evaluation_times`` (:266-297), then sampling.

Inputs: a ``pulser_amd.hamiltonian_data.SequenceInputs`` (plain arrays; works
without pulser installed) or, when the user has pulser, a
``pulser.sampler.SequenceSamples`` + register + device / a ``pulser.Sequence``.
"""

from __future__ import annotations

import math
import os
import sys
import warnings
from collections import Counter
from dataclasses import dataclass, field
from enum import Enum
from functools import lru_cache
from typing import Any, Iterator, Optional, Union, cast

import numpy as np

from .hamiltonian_data import HamiltonianData, SequenceInputs
from .noise_model import (LEGACY_DEFAULTS, NoiseModel, _NOISE_TYPE_PARAMS,
                          check_eff_noise, has_stochastic_noise)
from .results import (DeviceState, CoherentResults, EnsembleState, LazyState, NoisyResults, QState, SampledResult,
                      SimulationResults, SnapshotStore, StateResult, operator_key)
from .terms import sampling_times

__all__ = ["QutipEmulator", "Solver", "SimConfig", "NoiseModel"]


class Solver(str, Enum):
    """simulation.py:67-81.  DEFAULT picks the Schroedinger or master-equation
    kernels from the noise model; MCSOLVER runs quantum-jump trajectories."""

    DEFAULT = "default"
    MESOLVER = "MasterEquation"
    MCSOLVER = "MonteCarlo"


_DIFF_NOISE_PARAMS = {
    "noise_types": "noise",
    "state_prep_error": "eta",
    "p_false_pos": "epsilon",
    "p_false_neg": "epsilon_prime",
}


def _find_relevant_params(noise_types, state_prep_error, amp_sigma, laser_waist) -> set[str]:
    """pulser-core/pulser/noise_model.py:497-520."""
    relevant: set[str] = set()
    for nt in noise_types:
        relevant.update(_NOISE_TYPE_PARAMS[nt])
        if nt == "register":
            relevant.add("temperature")
        if (nt in ("doppler", "detuning", "register", "dmm_sigma")
                or (nt == "amplitude" and amp_sigma != 0.0)
                or (nt == "SPAM" and state_prep_error != 0.0)):
            relevant.update(("runs", "samples_per_run"))
    if laser_waist is None:
        relevant.discard("laser_waist")
    return relevant


@dataclass(frozen=True)
class SimConfig:
    """Deprecated configuration shim (pulser_simulation/simconfig.py:42-157):
    converts to / from a ``NoiseModel``."""

    noise: Union[str, tuple] = ()
    runs: int = LEGACY_DEFAULTS["runs"]
    samples_per_run: int = LEGACY_DEFAULTS["samples_per_run"]
    temperature: float = LEGACY_DEFAULTS["temperature"]
    laser_waist: float = LEGACY_DEFAULTS["laser_waist"]
    amp_sigma: float = LEGACY_DEFAULTS["amp_sigma"]
    detuning_sigma: float = 0.0
    eta: float = LEGACY_DEFAULTS["state_prep_error"]
    epsilon: float = LEGACY_DEFAULTS["p_false_pos"]
    epsilon_prime: float = LEGACY_DEFAULTS["p_false_neg"]
    relaxation_rate: float = LEGACY_DEFAULTS["relaxation_rate"]
    dephasing_rate: float = LEGACY_DEFAULTS["dephasing_rate"]
    hyperfine_dephasing_rate: float = LEGACY_DEFAULTS["hyperfine_dephasing_rate"]
    depolarizing_rate: float = LEGACY_DEFAULTS["depolarizing_rate"]
    eff_noise_rates: list = field(default_factory=list, repr=False)
    eff_noise_opers: list = field(default_factory=list, repr=False)
    solver_options: dict | None = None

    def __post_init__(self) -> None:
        warnings.warn(
            "'SimConfig' has been deprecated since v1.6 and will be removed in a "
            "future version. Please use 'NoiseModel' instead.",
            DeprecationWarning,
            stacklevel=3,
        )
        noise = (self.noise,) if isinstance(self.noise, str) else tuple(self.noise)
        object.__setattr__(self, "noise", noise)
        if not isinstance(self.temperature, (int, float)):
            raise TypeError(f"'temperature' must be a float, not {type(self.temperature)}.")
        # temperature is given in uK and stored in K (simconfig.py:166)
        object.__setattr__(self, "temperature", self.temperature / 1e6)
        unknown = set(noise) - set(_NOISE_TYPE_PARAMS)
        if unknown:
            raise ValueError(f"'{sorted(unknown)[0]}' is not a valid noise type.")
        for param, value in self.spam_dict.items():  # simconfig.py:242-248
            if value > 1 or value < 0:
                raise ValueError(f"SPAM parameter {param} = {value} must be"
                                 + " greater than 0 and less than 1.")
        for operator in self.eff_noise_opers:  # simconfig.py:253-268
            if not isinstance(operator, np.ndarray) and not hasattr(operator, "full"):
                raise TypeError(f"{operator} is not a matrix (NumPy array or Qobj).")
            if np.asarray(operator).ndim != 2 or np.asarray(operator).shape[0] != np.asarray(operator).shape[1]:
                raise TypeError("Operators are supposed to be square matrices (Qutip type 'oper').")
        check_eff_noise(self.eff_noise_rates, [np.asarray(o) for o in self.eff_noise_opers],
                        "eff_noise" in noise, self.with_leakage)

    @property
    def with_leakage(self) -> bool:
        return "leakage" in self.noise

    @property
    def spam_dict(self) -> dict[str, float]:
        return {"eta": self.eta, "epsilon": self.epsilon, "epsilon_prime": self.epsilon_prime}

    @property
    def doppler_sigma(self) -> float:
        from .noise_model import doppler_sigma

        return doppler_sigma(self.temperature)

    @property
    def supported_noises(self) -> dict:
        from .hamiltonian_data import SUPPORTED_NOISES

        return SUPPORTED_NOISES

    def __str__(self, solver_options: bool = False) -> str:
        """simconfig.py:204-240."""
        lines = [
            "Options:",
            "----------",
            f"Number of runs:        {self.runs}",
            f"Samples per run:       {self.samples_per_run}",
        ]
        if self.noise:
            lines.append("Noise types:           " + ", ".join(self.noise))
        if "SPAM" in self.noise:
            lines.append(f"SPAM dictionary:       {self.spam_dict}")
        if "eff_noise" in self.noise:
            lines.append(f"Effective noise rates:       {self.eff_noise_rates}")
            lines.append(f"Effective noise operators:       {self.eff_noise_opers}")
        if "doppler" in self.noise:
            lines.append(f"Temperature:           {self.temperature*1.e6}µK")
        if "amplitude" in self.noise:
            lines.append(f"Laser waist:           {self.laser_waist}μm")
            lines.append(f"Amplitude standard dev.:  {self.amp_sigma}")
        if "relaxation" in self.noise:
            lines.append(f"Relaxation rate: {self.relaxation_rate}")
        if "dephasing" in self.noise:
            lines.append(f"Dephasing rate: {self.dephasing_rate} (Rydberg), "
                         f"{self.hyperfine_dephasing_rate} (Hyperfine)")
        if "depolarizing" in self.noise:
            lines.append(f"Depolarizing rate: {self.depolarizing_rate}")
        if solver_options:
            lines.append("Solver Options: \n" + f"{str(self.solver_options)[10:-1]}")
        return "\n".join(lines).rstrip()

    @classmethod
    def from_noise_model(cls, noise_model: Any) -> "SimConfig":
        kwargs: dict[str, Any] = dict(noise=noise_model.noise_types)
        for param in _find_relevant_params(noise_model.noise_types, noise_model.state_prep_error,
                                           noise_model.amp_sigma, noise_model.laser_waist):
            kwargs[_DIFF_NOISE_PARAMS.get(param, param)] = getattr(noise_model, param)
        if "amplitude" in noise_model.noise_types:
            kwargs.setdefault("laser_waist", float("inf"))
        kwargs.pop("with_leakage", None)
        if kwargs.get("runs", 0) is None:
            kwargs.pop("runs")
        for k in ("detuning_hf_psd", "detuning_hf_omegas", "trap_waist", "trap_depth",
                  "dmm_sigma", "detuning_map_spot_waist"):
            kwargs.pop(k, None)
        if "eff_noise_opers" in kwargs:
            kwargs["eff_noise_opers"] = [np.array(o) for o in kwargs["eff_noise_opers"]]
            kwargs["eff_noise_rates"] = list(kwargs.get("eff_noise_rates", []))
        return cls(**kwargs)

    def to_noise_model(self) -> NoiseModel:
        laser_waist_ = None if math.isinf(self.laser_waist) else self.laser_waist
        kwargs = {}
        for param in _find_relevant_params(self.noise, self.eta, self.amp_sigma, laser_waist_):
            kwargs[param] = getattr(self, _DIFF_NOISE_PARAMS.get(param, param))
        if "temperature" in kwargs:
            kwargs["temperature"] *= 1e6
        if "eff_noise_opers" in kwargs:
            kwargs["eff_noise_opers"] = tuple(np.array(o) for o in kwargs["eff_noise_opers"])
            kwargs["eff_noise_rates"] = tuple(kwargs["eff_noise_rates"])
        return NoiseModel(**kwargs)


def _env_window_knots(default: int = 32) -> int:
    """PULSER_AMD_WINDOW_KNOTS (knots per evaluation-time window): an integer >= 2; anything else gives the default and a
    warning, like the native side's out-of-range RYD_* values (dev_common.hpp: dev_env_int)."""
    env = os.environ.get("PULSER_AMD_WINDOW_KNOTS")
    if env is None:
        return default
    try:
        m = int(env)
    except ValueError:
        m = 0
    if m < 2:
        warnings.warn(f"PULSER_AMD_WINDOW_KNOTS={env!r} is not an integer >= 2; using {default}", stacklevel=2)
        return default
    return m


def _as_inputs(sampled_seq: Any, register: Any, device: Any) -> SequenceInputs:
    if isinstance(sampled_seq, SequenceInputs):
        return sampled_seq
    if hasattr(sampled_seq, "samples_list") and hasattr(sampled_seq, "channels"):
        from .pulser_adapter import sequence_inputs_from_pulser

        return sequence_inputs_from_pulser(sampled_seq, register, device)
    raise TypeError("The provided sequence has to be a valid SequenceSamples instance.")


class _EnsembleSums:
    """The running sums over the trajectories of an ensemble route (``run(mc_ensemble=True)``): what ``observe_many``
    returns per trajectory - ``[T', B, ...]`` host arrays, not normalised - summed over the trajectory axis per local
    state counted (``digits``; the two-level kernels count local state 0), with the squared occupations for the
    standard error; :meth:`states` turns them into one ``EnsembleState`` per evaluation time.

    ``n_targets`` / ``operators`` (``run(mc_ensemble_targets=..., mc_ensemble_operators=...)``; the ``operator_key`` of
    every operator): :meth:`add_overlaps` sums what ``overlap_many`` and ``expect_sparse`` return per trajectory -
    ``|z_b|^2`` and its square, ``e_b`` and the squares of its two parts - for ``fidelity`` / ``expectation`` and their
    standard errors."""

    def __init__(self, n_times: int, n_qudits: int, digits: Any = (0,), n_targets: int = 0,
                 operators: Any = ()) -> None:
        self.digits = tuple(digits)
        self._n_times = int(n_times)
        self._sums: dict[int, dict[str, np.ndarray]] = {d: {} for d in self.digits}
        self._occ_sq = {d: np.zeros((self._n_times, n_qudits)) for d in self.digits}
        self._operators = tuple(operators)
        self._fid = np.zeros((self._n_times, int(n_targets)))  # sum_b |z_b|^2
        self._fid_sq = np.zeros_like(self._fid)  # sum_b |z_b|^4
        self._exp = np.zeros((self._n_times, len(self._operators)), dtype=np.complex128)  # sum_b e_b
        self._exp_sq = np.zeros(self._exp.shape + (2,))  # sum_b (Re e_b)^2, sum_b (Im e_b)^2

    def add(self, rows: dict[str, np.ndarray], at: slice, weight: int = 1, digit: int | None = None) -> None:
        """Add the rows of the evaluation times ``at``, each trajectory ``weight`` times (``digit``: the first one)."""
        digit = self.digits[0] if digit is None else digit
        sums = self._sums[digit]
        for k, v in rows.items():
            if k not in sums:
                sums[k] = np.zeros((self._n_times,) + tuple(v.shape[2:]))
            sums[k][at] += weight * v.sum(axis=1)
        self._occ_sq[digit][at] += weight * (rows["occupation"] ** 2).sum(axis=1)

    def add_overlaps(self, z: np.ndarray, e: np.ndarray, at: slice, weight: int = 1) -> None:
        """Add the overlaps ``z`` complex[T', B, F] with the targets and the expectation values ``e`` complex[T', B, K]
        of the operators at the evaluation times ``at``, each trajectory ``weight`` times."""
        p = z.real * z.real + z.imag * z.imag
        self._fid[at] += weight * p.sum(axis=1)
        self._fid_sq[at] += weight * (p * p).sum(axis=1)
        self._exp[at] += weight * e.sum(axis=1)
        self._exp_sq[at] += weight * np.stack([(e.real * e.real).sum(axis=1), (e.imag * e.imag).sum(axis=1)], axis=-1)

    @staticmethod
    def _variance(sum_sq: np.ndarray, mean: np.ndarray, ntraj: int) -> np.ndarray:
        """The sample variance (ddof = 1) [T, ...] of values with the sum of squares ``sum_sq`` and the mean ``mean``:
        nan for one trajectory, exactly 0 at the first evaluation time."""
        if ntraj <= 1:  # (one trajectory has no sample deviation)
            return np.full_like(sum_sq, np.nan)
        var = np.maximum(sum_sq - ntraj * mean ** 2, 0.0) / (ntraj - 1)
        var[0] = 0.0  # every trajectory starts in the same ket (not left to the rounding of sum x^2 - n mean^2)
        return var

    def _means(self, digit: int, ntraj: int) -> dict[str, np.ndarray]:
        """Trajectory means of the pair sums of ``digit`` [T, ...] and the standard error of its occupations."""
        sums, occ_sq = self._sums[digit], self._occ_sq[digit]
        mean_occ = sums["occupation"] / ntraj
        stderr = np.sqrt(self._variance(occ_sq, mean_occ, ntraj) / ntraj)
        return {"occupation": mean_occ, "correlation": sums["correlation"] / ntraj, "occupation_stderr": stderr}

    def _overlap_means(self, ntraj: int) -> dict[str, np.ndarray]:
        """Trajectory means of what :meth:`add_overlaps` summed [T, F] / [T, K] and their standard errors."""
        fid, exp = self._fid / ntraj, self._exp / ntraj
        var = self._variance(self._exp_sq[..., 0], exp.real, ntraj) + self._variance(self._exp_sq[..., 1], exp.imag, ntraj)
        return {"fidelity": fid, "fidelity_stderr": np.sqrt(self._variance(self._fid_sq, fid, ntraj) / ntraj),
                "expectation": exp, "expectation_stderr": np.sqrt(var / ntraj)}

    def states(self, diag_sums: np.ndarray, ntraj: int, with_energy: bool = True,
               by_digit: bool = False, subsystems: Any = (), reduced_sums: Any = ()) -> list[EnsembleState]:
        """One ``EnsembleState`` per evaluation time from the summed diagonals ``diag_sums`` [T, D]; the norm and the
        energy moments are those that came with the first digit (``with_energy=False``: nan).  ``by_digit``: the
        states carry the means of every digit, else those of the first one as plain attributes.  ``subsystems`` /
        ``reduced_sums`` (``run(mc_ensemble_subsystems=...)``): site tuples and, for each, the trajectory sums
        ``[T, dA, dA]`` of its reduced density matrices."""
        means = {d: self._means(d, ntraj) for d in self.digits}
        lead, first = self._sums[self.digits[0]], means[self.digits[0]]
        overlaps = self._overlap_means(ntraj)
        out = []
        for i in range(self._n_times):
            pairs: dict[str, Any] = (
                {"by_digit": {d: {k: v[i] for k, v in m.items()} for d, m in means.items()}} if by_digit
                else {k: v[i] for k, v in first.items()})
            pairs.update({k: v[i] for k, v in overlaps.items()}, operators=self._operators)
            if len(subsystems):
                pairs.update(subsystems=subsystems, reduced=[r[i] for r in reduced_sums])
            out.append(EnsembleState(diag_sums[i], ntraj, norm2=lead["norm2"][i] / ntraj,
                                     energy=lead["energy"][i] / ntraj if with_energy else math.nan,
                                     energy2=lead["energy2"][i] / ntraj if with_energy else math.nan, **pairs))
        return out


class QutipEmulator:
    """Emulator of a pulse sequence on MI355X (drop-in for
    ``pulser_simulation.QutipEmulator``; arguments as simulation.py:130-141)."""

    def __init__(
        self,
        sampled_seq: Any,
        register: Any = None,
        device: Any = None,
        sampling_rate: float = 1.0,
        config: Optional[SimConfig] = None,
        evaluation_times: Union[float, str, Any] = "Full",
        noise_model: Any = None,
        solver: Solver = Solver.DEFAULT,
        n_trajectories: int | None = None,
    ) -> None:
        samples = _as_inputs(sampled_seq, register, device)
        if samples.max_duration == 0:
            raise ValueError("SequenceSamples is empty.")
        self._sampling_rate = sampling_rate
        self.solver = Solver(solver)
        self._tot_duration = samples.max_duration
        self.samples_obj = samples.extend_duration(self._tot_duration + 1)  # :173
        self._n_trajectories = n_trajectories
        if not (0 < sampling_rate <= 1.0):
            raise ValueError(
                "The sampling rate (`sampling_rate` = "
                f"{sampling_rate}) must be greater than 0 and "
                "less than or equal to 1."
            )
        if int(self._tot_duration * sampling_rate) < 4:
            raise ValueError("`sampling_rate` is too small, less than 4 data points.")
        if noise_model is not None and config is not None:
            raise ValueError(
                "'noise_model' and 'config' cannot both be provided to "
                "'QutipEmulator'. Please provide just a 'noise_model'."
            )
        if config is not None:
            warnings.warn(
                "Supplying a 'SimConfig' to QutipEmulator has been "
                "deprecated. Please instantiate with a 'NoiseModel' instead.",
                DeprecationWarning,
                stacklevel=2,
            )
            noise_model = config.to_noise_model()
        if not noise_model:
            noise_model = NoiseModel()
        self._noise_trajectories_used = False
        self._hamiltonian_data = HamiltonianData(
            self.samples_obj, noise_model,
            self._get_n_trajectories(noise_model, check_value=True),
        )
        self._problems_cache: list[dict[str, Any]] | None = None
        self._current_problem = self._hamiltonian_data.problem(
            self._hamiltonian_data.noise_trajectories[0], self._sampling_rate)
        self._eval_times_array: np.ndarray
        self.set_evaluation_times(evaluation_times)
        if self.samples_obj.measurement:
            self._meas_basis = self.samples_obj.measurement
        elif "all" in self.basis_name:
            self._meas_basis = "digital"
        else:
            self._meas_basis = self.basis_name.replace("_with_error", "")
        self.set_initial_state("all-ground")
        self._engine_opts: dict[str, Any] = {}
        self.last_engine_stats: dict[str, Any] = {}

    # ------------------------------------------------------------------ setup
    @property
    def _problems(self) -> list[dict[str, Any]]:
        """Problem bundles of every trajectory (materialised on first use; the
        stochastic run path lowers trajectories in factored form instead)."""
        if self._problems_cache is None:
            self._problems_cache = list(self._hamiltonian_data.problems(self._sampling_rate))
        return self._problems_cache

    @_problems.setter
    def _problems(self, value: list[dict[str, Any]]) -> None:
        self._problems_cache = value

    def _get_n_trajectories(self, noise_model: Any, check_value: bool) -> int | None:
        n = self._n_trajectories if self._n_trajectories is not None else noise_model.runs
        if check_value and has_stochastic_noise(noise_model) and n is None:
            raise ValueError(
                "'n_trajectories' must be defined when the NoiseModel contains"
                " stochastic noise, which is the case for the given noise "
                f"model: {noise_model!r}"
            )
        return n

    @property
    def n_trajectories(self) -> int | None:
        return self._get_n_trajectories(self.noise_model, check_value=False)

    @lru_cache(maxsize=2)
    def _get_noiseless_data(self, leakage: bool) -> HamiltonianData:
        """simulation.py:266-297: a second HamiltonianData (draws RNG once)."""
        if leakage:
            noise = NoiseModel(eff_noise_opers=(np.zeros((3, 3)),), eff_noise_rates=(0.0,),
                               with_leakage=True)
        else:
            noise = NoiseModel()
        return HamiltonianData(self.samples_obj, noise, n_trajectories=1)

    @property
    def _noiseless_problem(self) -> dict[str, Any]:
        hd = self._get_noiseless_data(False)
        return hd.problem(hd.noise_trajectories[0], self._sampling_rate)

    @property
    def sampling_times(self) -> np.ndarray:
        self._get_noiseless_data(False)
        return sampling_times(self.samples_obj.max_duration, self._sampling_rate)

    @property
    def dim(self) -> int:
        return len(self._hamiltonian_data.eigenbasis)

    @property
    def basis_name(self) -> str:
        return self._hamiltonian_data.basis_name

    @property
    def basis(self) -> dict[str, QState]:
        eb = self._hamiltonian_data.eigenbasis
        return {s: QState(np.eye(len(eb))[i]) for i, s in enumerate(eb)}

    @property
    def noise_model(self) -> Any:
        return self._hamiltonian_data.noise_model

    @property
    def config(self) -> SimConfig:
        return SimConfig.from_noise_model(self._hamiltonian_data.noise_model)

    @property
    def total_duration_ns(self) -> int:
        return self._tot_duration

    # -- deprecated SimConfig surface (simulation.py:348-476) -------------------
    # Same contract as the reference (warnings, exception types and messages, the
    # all-ground fallback when the level structure changes); the mechanics are ours:
    # one validator shared by set / add, and the merge is done on NoiseModel fields.
    def _check_legacy_config(self, candidate: Any, *, colon_space: bool, period: bool) -> NoiseModel:
        """Deprecation notice + the two rejections of the legacy entry points; returns the
        candidate as a NoiseModel.  (The reference's two messages differ by a space after
        the colon and a trailing period; both are asserted by its tests.)"""
        warnings.warn(
            "Supplying a 'SimConfig' to QutipEmulator has been deprecated."
            " Please instantiate with a 'NoiseModel' instead.",
            DeprecationWarning,
            stacklevel=3,
        )
        if not isinstance(candidate, SimConfig):
            raise ValueError(f"Object {candidate} is not a valid `SimConfig`" + ("." if period else ""))
        mode = self._hamiltonian_data.interaction_type
        refused = [kind for kind in candidate.noise if kind not in candidate.supported_noises[mode]]
        if refused:
            raise NotImplementedError(
                f"Interaction mode '{mode}' does not support simulation of noise types:"
                + (" " if colon_space else "") + ", ".join(refused) + "."
            )
        return candidate.to_noise_model()

    def _install_noise_model(self, model: NoiseModel) -> None:
        """Swap the noise model: fresh trajectory draws, caches dropped, and the initial
        state carried over when the local dimension is unchanged."""
        dim_before, ground_before = self.dim, np.asarray(self._all_ground())
        self._noise_trajectories_used = False
        self._problems_cache = None
        self._hamiltonian_data = HamiltonianData(
            self.samples_obj, model, self._get_n_trajectories(model, check_value=True))
        first = self._hamiltonian_data.noise_trajectories[0]
        self._current_problem = self._hamiltonian_data.problem(first, self._sampling_rate)
        kept = np.asarray(self._initial_state)
        if self.dim == dim_before:
            self.set_initial_state(kept)
        else:
            if not np.array_equal(kept, ground_before):
                warnings.warn(
                    "Current initial state's dimension does not match new"
                    " dimensions. Setting it to 'all-ground'."
                )
            self.set_initial_state("all-ground")

    def set_config(self, cfg: SimConfig) -> None:
        """Replace the noise configuration."""
        self._install_noise_model(self._check_legacy_config(cfg, colon_space=False, period=True))

    def add_config(self, config: SimConfig) -> None:
        """Merge another configuration into the current one: only the noise types that
        are NEW bring their parameters; for types present in both the current values stay."""
        incoming = self._check_legacy_config(config, colon_space=True, period=False)
        present = self._hamiltonian_data.noise_model
        fresh_types = set(incoming.noise_types).difference(present.noise_types)
        adopted = _find_relevant_params(fresh_types, incoming.state_prep_error,
                                        incoming.amp_sigma, incoming.laser_waist)
        import dataclasses

        fields = {f.name: getattr(present, f.name) for f in dataclasses.fields(present)
                  if f.name != "noise_types"}
        fields.update({name: getattr(incoming, name) for name in adopted})
        # through SimConfig, as the reference does: its field set (and defaults) decide what survives
        self._install_noise_model(SimConfig.from_noise_model(NoiseModel(**fields)).to_noise_model())

    def show_config(self, solver_options: bool = False) -> None:
        """Prints the current configuration."""
        print(self.config.__str__(solver_options))

    def reset_config(self) -> None:
        """Back to the default (noiseless) configuration."""
        self._install_noise_model(SimConfig().to_noise_model())

    def draw(self, draw_phase_area: bool = False, draw_phase_shifts: bool = False,
             draw_phase_curve: bool = False, fig_name: str | None = None,
             kwargs_savefig: dict = {}) -> None:
        """Plots the samples the simulation uses, one panel per channel
        (simulation.py:917-953; the reference delegates to pulser's sequence
        drawer - this is the plain-matplotlib equivalent of its amplitude /
        detuning curves)."""
        import matplotlib.pyplot as plt

        chans = self.samples_obj.channels
        fig, axes = plt.subplots(len(chans), 1, sharex=True, squeeze=False,
                                 figsize=(8, 2.2 * len(chans)))
        t = np.arange(self.samples_obj.max_duration)
        for ax, ch in zip(axes[:, 0], chans):
            ax.plot(t, ch.amp, color="darkgreen", label="amplitude (rad/µs)")
            ax.plot(t, ch.det, color="indigo", label="detuning (rad/µs)")
            if draw_phase_curve and np.any(np.diff(ch.phase)):
                ax.plot(t, ch.phase, color="gray", ls=":", label="phase (rad)")
            ax.set_ylabel(ch.name)
            ax.legend(loc="upper right", fontsize=7)
        axes[-1, 0].set_xlabel("t (ns)")
        if fig_name is not None:
            plt.savefig(fig_name, **kwargs_savefig)
        plt.show()

    @property
    def initial_state(self) -> QState:
        return self._initial_state

    def _all_ground(self) -> QState:
        eb = self._hamiltonian_data.eigenbasis
        v = "u" if self._hamiltonian_data.interaction_type == "XY" else "g"
        loc = eb.index(v)
        idx = 0
        for _ in range(self._hamiltonian_data.n_qudits):
            idx = idx * len(eb) + loc
        psi = np.zeros(len(eb) ** self._hamiltonian_data.n_qudits, dtype=complex)
        psi[idx] = 1.0
        return QState(psi)

    def set_initial_state(self, state: Any) -> None:
        """simulation.py:484-525."""
        if isinstance(state, str) and state == "all-ground":
            self._initial_state = self._all_ground()
            self._initial_is_ground = True
            return
        arr = np.asarray(state)
        shape = arr.shape[0]
        legal_shape = self.dim ** self._hamiltonian_data.n_qudits
        if shape != legal_shape:
            raise ValueError(
                "Incompatible shape of initial state."
                + f"Expected {legal_shape}, got {shape}."
            )
        if arr.ndim > 1 and int(np.prod(arr.shape[1:])) != 1:
            # the reference builds qutip.Qobj(state, dims=[[d] * N, [1] * N]) (simulation.py:519-529): ket dimensions - a
            # density matrix (or any matrix) does not fit them and qutip raises.  Same here, instead of flattening D x D
            # numbers into a "ket" ("missing" item 3: the reference does not accept operators either)
            raise ValueError(
                "Incompatible shape of initial state: the initial state is a ket "
                f"(dims [[{self.dim}] * {self._hamiltonian_data.n_qudits}, [1] * {self._hamiltonian_data.n_qudits}]), "
                f"got an array of shape {arr.shape}."
            )
        self._initial_state = QState(arr.reshape(-1)).unit()
        self._initial_is_ground = bool(
            np.array_equal(np.asarray(self._initial_state), np.asarray(self._all_ground()))
        )

    @property
    def evaluation_times(self) -> np.ndarray:
        return np.array(self._eval_times_array)

    _EVAL_LABEL_ERROR = ("Wrong evaluation time label. It should be `Full`, `Minimal`, an array of times or a "
                         "float between 0 and 1.")

    def _requested_times(self, spec: Any) -> np.ndarray:
        """The times (us) a specification asks for, before the end points are added.  A table of
        the accepted kinds; everything else is a label error (contract of simulation.py:532-599)."""
        grid = self.sampling_times
        t_end = self._tot_duration * 1e-3
        if isinstance(spec, str):
            named = {"Full": lambda: grid.copy(), "Minimal": lambda: np.empty(0)}
            if spec not in named:
                raise ValueError(self._EVAL_LABEL_ERROR)
            return named[spec]()
        if isinstance(spec, float):  # a fraction of the sampling grid, evenly thinned
            if not 0 < spec <= 1:
                raise ValueError("evaluation_times float must be between 0 and 1.")
            keep = np.linspace(0, grid.size - 1, int(spec * grid.size), dtype=int)
            return grid[keep]
        if isinstance(spec, (list, tuple, np.ndarray)):
            times = np.array(spec)
            if times.size:
                if times.max() > t_end and times.max() > 0:
                    raise ValueError("Provided evaluation-time list extends further than sequence duration.")
                if times.min() < 0:
                    raise ValueError("Provided evaluation-time list contains negative values.")
            return times
        raise ValueError(self._EVAL_LABEL_ERROR)

    def set_evaluation_times(self, value: Any) -> None:
        """Evaluation times always contain 0 and the end of the sequence (simulation.py:596-598)."""
        asked = self._requested_times(value)
        self._eval_times_array = np.union1d(asked, [0.0, self._tot_duration * 1e-3])
        self._eval_times_instruction = value

    # --------------------------------------------------------------- operators
    def build_operator(self, operations: Union[list, tuple]) -> np.ndarray:
        """Dense operator from ``[(op, qubits), ...]`` (hamiltonian.py:145-200)."""
        eb = self._hamiltonian_data.eigenbasis
        d, n = len(eb), self._hamiltonian_data.n_qudits
        ops = {"I": np.eye(d, dtype=complex)}
        for i, a in enumerate(eb):
            for j, b in enumerate(eb):
                m = np.zeros((d, d), dtype=complex)
                m[i, j] = 1
                ops["sigma_" + a + b] = m
        if not isinstance(operations, list):
            operations = [operations]
        qids = list(self.samples_obj.qubit_ids)
        op_list = [ops["I"]] * n
        for operator, qubits in operations:
            if isinstance(operator, str):
                if operator not in ops:
                    raise ValueError(f"{operator} is not a valid operator")
                operator = ops[operator]
            operator = np.asarray(operator, dtype=complex)
            if qubits == "global":
                return sum(self.build_operator([(operator, [q])]) for q in qids)
            if len(set(qubits)) < len(qubits):
                raise ValueError("Duplicate atom ids in argument list.")
            if not set(qubits).issubset(qids):
                raise ValueError("Invalid qubit names: " f"{set(qubits) - set(qids)}")
            for q in qubits:
                op_list[qids.index(q)] = operator
        out = np.eye(1, dtype=complex)
        for m in op_list:
            out = np.kron(out, m)
        return out

    def get_hamiltonian(self, time: float, noiseless: bool = False) -> np.ndarray:
        """Dense H(t) in rad/us at ``time`` ns (simulation.py:625-661); built by
        applying the device generator to the identity (small registers only)."""
        if time > self._tot_duration:
            raise ValueError(
                f"Provided time (`time` = {time}) must be "
                "less than or equal to the sequence duration "
                f"({self._tot_duration})."
            )
        if time < 0:
            raise ValueError(
                f"Provided time (`time` = {time}) must be greater than or equal to 0."
            )
        from .engine import Engine, GeneralEngine
        from .general import lower_general

        prob = dict(self._noiseless_problem if noiseless else self._current_problem)
        prob["collapse_ops"] = []
        n = prob["n_qudits"]
        D = len(prob["eigenbasis"]) ** n
        if D > 4096:
            raise ValueError("get_hamiltonian materialises a dense matrix; at most 4096 states.")
        cols = np.zeros((D, D), dtype=complex)
        ctx = (Engine.from_problems([prob], mode="sesolve") if self._fast_path_ok(prob)
               else GeneralEngine(lower_general(prob, mesolve=False)))
        with ctx as eng:
            import torch

            for j in range(D):
                e = torch.zeros((1, D), dtype=torch.complex128, device=eng.device)
                e[0, j] = 1.0
                cols[:, j] = eng.apply_generator(e, time / 1000).cpu().numpy()[0]
        return QState(1j * cols)  # G = -iH, column j = G e_j

    # --------------------------------------------------------------------- run
    def _validate_options(self, options: dict[str, Any]) -> None:
        """simulation.py:768-797."""

        def min_variation(ch: Any) -> int:  # simulation.py:663-687
            end_point = ch.duration - 1
            mins = []
            for sample in (np.asarray(ch.amp), np.asarray(ch.det)):
                mins.append(int(np.min(np.diff(np.nonzero(np.diff(sample)), prepend=-1,
                                               append=end_point))))
            return min(mins)

        self._mc_rng = None  # a new run restarts the jump-seed generator (option ``seeds``)
        # the reference's DEFAULT max_step (shortest waveform variation) keeps QuTiP's adaptive ODE solver
        # from stepping over pulse features; the CF4 stepper never steps over a spline knot that matters
        # (it merges knots only where the waveform is the same polynomial on both sides), so only a
        # max_step the caller asked for is handed to the engine
        # (validate a dict ONCE: a second pass would see the filled-in default as a request;
        # run_ensemble(options_validated=True) when run() hands its options on)
        self._default_max_step = "max_step" not in options
        options.setdefault(
            "max_step", min(min_variation(ch) for ch in self.samples_obj.channels) / 1000
        )
        options.setdefault("nsteps", max(1000, self._tot_duration // options["max_step"]))
        if "SPAM" in self.noise_model.noise_types:
            if self.noise_model.state_prep_error > 0 and not self._initial_is_ground:
                raise NotImplementedError(
                    "Can't combine state preparation errors with an initial "
                    "state different from the ground."
                )
        if options.get("mc_ensemble_targets") is not None or options.get("mc_ensemble_operators") is not None:
            self._ensemble_observables(options)  # (a ValueError here: nothing is solved)
        if options.get("mc_ensemble_subsystems") is not None:
            self._ensemble_subsystems(options)  # (the same)

    def _ensemble_subsystems(self, options: dict[str, Any]) -> list[tuple[int, ...]]:
        """The option ``mc_ensemble_subsystems`` as sorted site tuples (positions in ``samples_obj.qubit_ids``);
        ``ValueError`` for an entry that is empty, holds something that is no integer, a duplicate or a site out of
        range, or makes more rows than the device partial trace serves (2^k <= 64)."""
        from .engine import REDUCED_DENSITY_MAX_ROWS, check_keep

        given = options.get("mc_ensemble_subsystems")
        n = self._hamiltonian_data.n_qudits
        out = []
        for k, item in enumerate([] if given is None else list(given)):
            try:
                sites = check_keep(item, n)
            except ValueError as exc:
                raise ValueError(f"mc_ensemble_subsystems[{k}]: {exc}") from None
            if 2 ** len(sites) > REDUCED_DENSITY_MAX_ROWS:
                raise ValueError(f"mc_ensemble_subsystems[{k}] holds {len(sites)} sites: the reduced density matrix "
                                 f"of an ensemble has at most {REDUCED_DENSITY_MAX_ROWS} rows (6 two-level atoms)")
            out.append(sites)
        return out

    def _ensemble_observables(self, options: dict[str, Any]) -> tuple[np.ndarray, list[Any]]:
        """The options ``mc_ensemble_targets`` / ``mc_ensemble_operators`` of an ensemble route as (the kets
        complex128[F, D], the operators as K complex128 CSR matrices [D, D] - duplicates summed, stored zeros dropped,
        sorted), D = d^N in the run's eigenbasis order; ``ValueError`` for anything else."""
        import scipy.sparse as sp

        D = self.dim ** self._hamiltonian_data.n_qudits
        given = options.get("mc_ensemble_targets")
        items = [] if given is None else list(given)
        targets = np.zeros((len(items), D), dtype=np.complex128)
        for f, item in enumerate(items):
            a = np.asarray(item)
            if a.dtype.kind not in "biufc":
                raise ValueError(f"mc_ensemble_targets[{f}] is not numeric (dtype {a.dtype})")
            if a.ndim == 2 and a.shape[0] == a.shape[1] and a.shape[0] > 1:
                raise ValueError(f"mc_ensemble_targets[{f}] is a matrix of shape {a.shape}: the ensemble route takes "
                                 "kets; a mixed target needs the default route (mc_ensemble=False)")
            if a.shape not in ((D,), (D, 1)):
                raise ValueError(f"mc_ensemble_targets[{f}] of shape {a.shape} is no ket of {D} amplitudes "
                                 f"([{D}] or [{D}, 1])")
            targets[f] = a.reshape(-1)
        given = options.get("mc_ensemble_operators")
        operators = []
        for k, item in enumerate([] if given is None else list(given)):
            m = SimulationResults._as_operator(item)
            if m.dtype.kind not in "biufc":
                raise ValueError(f"mc_ensemble_operators[{k}] is not numeric (dtype {m.dtype})")
            if tuple(m.shape) != (D, D):
                raise ValueError(f"mc_ensemble_operators[{k}] of shape {tuple(m.shape)}: expected {(D, D)}")
            c = sp.csr_matrix(m).astype(np.complex128)
            c.sum_duplicates()
            c.eliminate_zeros()
            c.sort_indices()
            operators.append(c)
        return targets, operators

    @staticmethod
    def _overlap_reducer(sums: _EnsembleSums, targets: np.ndarray, operators: list[Any], device: Any) -> Any:
        """``reduce(kets [T', B, D] on the device, at, weight=1)`` of an ensemble route: one ``overlap_many`` call with the
        targets and one ``expect_sparse`` call per operator over the ``T' B`` kets as one stack, summed into ``sums``
        (``_EnsembleSums.add_overlaps``).  The targets and the operators' non-zeros are uploaded here, once per run;
        with nothing registered nothing is launched."""
        from .engine import expect_sparse, overlap_many, sparse_triplets

        n_f, n_k, dim = len(targets), len(operators), int(targets.shape[1])
        if not n_f and not n_k:
            return lambda kets, at, weight=1: None
        import torch

        targets_dev = torch.from_numpy(targets).to(device) if n_f else None
        triplets = [sparse_triplets(m, dim, device) for m in operators]

        def reduce(kets: Any, at: slice, weight: int = 1) -> None:
            n_t, n_b = int(kets.shape[0]), int(kets.shape[1])
            flat = kets.reshape(n_t * n_b, dim)
            # (the norms that come with the overlaps are not needed: norm2 is observe_many's)
            z = overlap_many(flat, targets_dev)[0].cpu().numpy() if n_f else np.zeros((n_t * n_b, 0), dtype=complex)
            e = (torch.stack([expect_sparse(flat, t) for t in triplets], dim=1).cpu().numpy() if n_k
                 else np.zeros((n_t * n_b, 0), dtype=complex))
            sums.add_overlaps(z.reshape(n_t, n_b, n_f), e.reshape(n_t, n_b, n_k), at, weight)

        return reduce

    @staticmethod
    def _overlap_bytes(targets: np.ndarray, operators: list[Any], chunk: int) -> tuple[int, int]:
        """Device bytes of what :meth:`_overlap_reducer` keeps (per evaluation time: the overlaps and expectation
        values of one chunk; once per run: the targets and the operators' triplets), for the snapshot budget."""
        return (16 * chunk * (len(targets) + len(operators)),
                int(targets.nbytes) + sum(24 * int(m.nnz) for m in operators))

    def _solver_mode(self, problem: dict[str, Any]) -> str:
        """simulation.py:705-718."""
        if len(problem["collapse_ops"]) == 0:
            return "sesolve"
        if self.solver == Solver.DEFAULT:
            mode = "mcsolve" if has_stochastic_noise(self.noise_model) else "mesolve"
        else:
            mode = {Solver.MCSOLVER: "mcsolve", Solver.MESOLVER: "mesolve"}[self.solver]
        return mode

    @staticmethod
    def _mc_fast_ok(problem: dict[str, Any]) -> bool:
        """Quantum-jump trajectories run on the tuned ket kernels for 2-level
        Ising problems whose ``sum C^dag C`` is diagonal (every built-in noise
        channel).  Everything else that would take ``qutip.mcsolve`` is
        integrated with the master equation instead - the state ``mcsolve``
        samples in expectation."""
        from .terms import SUPPORTED_BASES, local_collapse_ops

        if problem["basis_name"] not in SUPPORTED_BASES or len(problem["eigenbasis"]) != 2:
            return False
        if problem.get("interaction_type") == "XY":
            return False
        c = local_collapse_ops(problem.get("collapse_ops", []), problem["eigenbasis"],
                               problem.get("depolarizing_pauli_2ds"))
        if c is None:
            return False
        m = sum(x.conj().T @ x for x in c)
        return bool(abs(m[0, 1]) <= 1e-13 * max(abs(m[0, 0]), abs(m[1, 1]), 1e-300)) and len(c) <= 16

    def _mc_seeds(self, n: int, options: dict[str, Any]) -> np.ndarray:
        """One 64-bit seed per quantum-jump trajectory.  Like ``qutip.mcsolve``
        (option ``seeds``) the jump randomness does not touch the global
        ``np.random`` stream that the noise trajectories and the sampling use."""
        override = getattr(self, "_mc_seed_override", None)
        if override is not None:  # multi-GPU ensembles: rank 0 drew the seeds of every trajectory
            sd = np.asarray(override, dtype=np.uint64)
            if sd.shape != (n,):
                raise ValueError(f"need {n} trajectory seeds, got {sd.shape}")
            return sd
        if getattr(self, "_mc_rng", None) is None:
            self._mc_rng = np.random.default_rng(options.get("seeds"))
        return self._mc_rng.integers(0, 2**64, size=n, dtype=np.uint64)

    def _engine_kwargs(self, options: dict[str, Any], general: bool = False) -> dict[str, Any]:
        """``general``: the explicit-term engine keeps the reference's default ``max_step`` too (tiny systems;
        the seeded golden Counters of the multi-level cases were captured with it)."""
        kw = {}
        for k in ("tol", "taylor_order", "max_order", "magnus_tol"):
            if k in options:
                kw[k] = options[k]
        if options.get("max_step") and (general or not getattr(self, "_default_max_step", False)):
            kw["max_step"] = float(options["max_step"])
        return kw

    # -- evaluation-time windows (round 6) -----------------------------------------------------------------------------
    # The reference's default, evaluation_times="Full", asks for the state at EVERY sampling time.  On the sequential path
    # every knot then ends a step - the 6-stage composition per knot, 20 634 stages for the 14-atom anneal where the same
    # sequence without intermediate states takes 5 618 - and a single sequence keeps ONE of the 256 CUs busy while it does
    # so.  The states between two times are independent of everything after them, so they are computed in parallel:
    # the main solve stores ANCHOR states every `_WINDOW_KNOTS` (32) knots (long sub-steps, as for "Minimal"), and ONE batched
    # solve then carries every anchor through the knots of its own window - n_windows kets on n_windows CUs, each with the
    # spline PIECES of the full sequence over its window (the tables are cut, never re-splined: a window's coefficients
    # are the full sequence's polynomials, bit for bit).  Errors of a window do not travel beyond it.  12 - 16 atoms (measured,
    # one sequence, warm: 12 atoms 80 -> 35 ms, 14: 213 -> 80, 16: 253 -> 146); PULSER_AMD_NO_WINDOWS=1 keeps the sequential path.
    # (measured at 14 atoms, main solve + window solve: 16 knots 67.3 + 3.7 ms, 32: 61.3 + 4.7, 64: 58.6 + 6.8; the variable: tuning probe only)
    _WINDOW_KNOTS = _env_window_knots()
    _WINDOW_TOL = 2e-11  # budget of a window solve = 500 x tol = 1e-8 (its error ends with the window)

    def _window_plan(self, tables: Any, mode: str, times: np.ndarray, kw: dict[str, Any]) -> Any:
        """(anchor indices, main evaluation indices) when the solve can take the windowed form, else None."""
        m = self._WINDOW_KNOTS
        n = self._hamiltonian_data.n_qudits
        if os.environ.get("PULSER_AMD_NO_WINDOWS") or mode != "sesolve" or not (12 <= n <= int(os.environ.get("PULSER_AMD_WINDOWS_MAX_ATOMS", "16"))):
            return None
        if tables.batch > 32 or tables.dterms is not None or len(times) < 4 * m:
            return None
        if any(k in kw for k in ("taylor_order", "max_order")):
            return None
        tk = np.asarray(tables.tknots, dtype=float)
        K = len(tk) - 1
        if K < 2 * m or len(times) < K + 1:
            return None
        dt = tk[1] - tk[0]
        if not (np.allclose(np.diff(tk), dt, rtol=0, atol=1e-12) and np.allclose(times[: K + 1], tk, rtol=0, atol=1e-12)):
            return None  # the evaluation times are not the spline knots themselves
        if kw.get("max_step") and float(kw["max_step"]) < dt * (1 - 1e-9):
            return None
        J = K // m                       # windows 0 .. J-1 start at knots 0, m, ..., (J-1) m and have all their m pieces
        anchors = np.arange(J + 1) * m
        main = np.concatenate([anchors, np.arange(anchors[-1] + 1, len(times))]).astype(np.int64)
        try:
            import torch

            free, _ = torch.cuda.mem_get_info()
            if 3.0 * 16 * (2**n) * tables.batch * len(times) > free:
                return None
        except Exception:  # pragma: no cover
            return None
        return anchors, main

    @staticmethod
    def _window_tables(tables: Any, anchors: np.ndarray, m: int) -> Any:
        """DeviceTables of the batch (sequence b, window j) -> entry b * J + j: the pieces [a_j, a_j + m) of every series
        as series of their own over the knots 0 .. m (relative time), descriptors re-pointed."""
        import dataclasses

        J = len(anchors) - 1
        n_ser = tables.pp.shape[0]
        pp = np.empty((n_ser * J, m, 4), dtype=np.complex128)
        for j in range(J):
            pp[j::J] = tables.pp[:, anchors[j]: anchors[j] + m, :]   # series s of window j -> id s * J + j
        desc = np.repeat(np.ascontiguousarray(tables.desc), J, axis=0)  # [B * J, n]: entry b * J + j
        shift = np.tile(np.arange(J, dtype=np.int32), tables.batch)[:, None]
        for f in ("drive_series", "det_series", "off_series"):
            ids = desc[f]
            desc[f] = np.where(ids >= 0, ids * J + shift, -1)
        inter = tables.interaction if tables.interaction.shape[0] == 1 else np.repeat(tables.interaction, J, axis=0)
        tk = np.asarray(tables.tknots, dtype=np.float64)
        return dataclasses.replace(
            tables, batch=tables.batch * J, tknots=np.ascontiguousarray(tk[: m + 1] - tk[0]), pp=pp, desc=desc,
            interaction=np.ascontiguousarray(inter), series_knots=[])

    def _solve_in_windows(self, eng: Any, tables: Any, state: Any, times: np.ndarray, kw: dict[str, Any],
                          plan: Any) -> tuple[Any, dict[str, Any]]:
        """The snapshots of ``eng.solve(state, times, store=True)`` - complex128[len(times) - 1, B, dim] - by anchors +
        windows (see above), and the engine statistics of both solves.  ``state`` ends as the final state, like ``solve``."""
        from .engine import Engine

        torch = eng.torch
        anchors, main = plan
        m, J, B = self._WINDOW_KNOTS, len(anchors) - 1, tables.batch
        timing = bool(os.environ.get("PULSER_AMD_WINDOW_TIMING"))
        marks: list[tuple[str, float]] = []

        def mark(label: str) -> None:
            if timing:
                import time as _time

                torch.cuda.synchronize()
                marks.append((label, _time.perf_counter()))

        mark("start")
        start = state.clone()
        snaps_main = eng.solve(state, times[main], store=True, **kw)            # [len(main) - 1, B, dim]
        mark("main solve")
        stats = eng.stats()
        # out[k - 1] = state at times[k].  The first J m slots seen as [J, m, B, dim]: row j holds the m - 1 knots inside
        # window j and, last, anchor j + 1; the tail (times behind the last anchor) follows
        out = torch.empty((len(times) - 1,) + tuple(snaps_main.shape[1:]), dtype=snaps_main.dtype, device=snaps_main.device)
        grid = out[: J * m].view((J, m) + tuple(out.shape[1:]))
        grid[:, m - 1] = snaps_main[:J]
        out[J * m:] = snaps_main[J:]
        # initial states of the windows: entry b * J + j = sequence b at anchor j
        init = torch.empty((B, J) + tuple(start.shape[1:]), dtype=start.dtype, device=start.device)
        init[:, 0] = start
        if J > 1:
            init[:, 1:] = snaps_main[: J - 1].transpose(0, 1)
        del start
        mark("anchors placed")
        wkw = dict(kw)
        # the budget of a solve is 500 x tol for its whole time span; a window's span is 32 knots, and its error ends with it:
        # a quarter of what the caller allowed the main solve, and never more than the default
        wkw["tol"] = min(self._WINDOW_TOL, 0.25 * float(kw["tol"])) if kw.get("tol") else self._WINDOW_TOL
        wt = self._window_tables(tables, anchors, m)
        mark("window tables")
        with Engine(wt, mode="sesolve") as weng:
            mark("window engine")
            wstate = init.reshape((B * J,) + tuple(init.shape[2:])).contiguous()
            del init
            wsnaps = weng.solve(wstate, np.asarray(wt.tknots[:m], dtype=np.float64), store=True, **wkw)  # [m - 1, B * J, dim]
            wstats = weng.stats()
            mark("window solve")
        # window j, knot i (i = 1 .. m - 1), sequence b: wsnaps[i - 1, b * J + j] -> grid[j, i - 1, b] (one strided copy)
        w = wsnaps.view((m - 1, B, J) + tuple(wsnaps.shape[2:]))
        grid[:, : m - 1] = w.permute(2, 0, 1, *range(3, w.dim()))
        del wsnaps, w
        mark("assembled")
        if timing:
            print("[windows] " + ", ".join(f"{b[0]} {1e3 * (b[1] - a[1]):.2f} ms" for a, b in zip(marks, marks[1:])), file=sys.stderr)
        # what the caller reads as the engine's statistics: both solves, the error estimates added (a state inside a
        # window carries the error of its anchor and of its window)
        merged = dict(stats)
        for k in ("n_applications", "n_launches", "n_steps"):
            merged[k] = stats[k] + wstats[k]
        merged["reserved"] = [stats["reserved"][0] + wstats["reserved"][0]] + list(stats["reserved"][1:])
        merged["windows"] = {"n_windows": B * J, "knots": m, "n_applications": wstats["n_applications"],
                             "n_launches": wstats["n_launches"], "estimate": wstats["reserved"][0]}
        return out, merged

    def _solve_batch(self, problems: list[dict[str, Any]], progress_bar: Any,
                     options: dict[str, Any], tables: Any = None,
                     mc_ntraj: int | None = None, raw: bool = False) -> Any:
        """The solver call of ``_run_solver`` (simulation.py:689-766) for a batch
        of trajectories in ONE engine (one GPU launch sequence).  ``tables``:
        pre-lowered device tables for the batch (factored noise) instead of
        ``problems``.  ``mc_ntraj``: the ``ntraj`` of ``qutip.mcsolve`` for the
        deterministic run (simulation.py:843); ``None`` = one quantum-jump
        trajectory per batch entry (the noisy runs, :726-727 with the default 1).
        ``raw`` (ensemble runs on pre-lowered ``tables``): nothing is wrapped - returns
        ``(initial_state_device [B, dim...], snapshots_device [n_eval - 1, B, dim...],
        occupations float64[n_eval, B, N + 1])`` with the occupations / norms reduced on the device
        (``ryd_occupations``), so that the caller can keep the state sums there too."""
        if progress_bar not in (True, False, None):
            raise ValueError("`progress_bar` must be a bool.")
        from .engine import Engine
        from .terms import lower

        if tables is None:
            mode = self._solver_mode(problems[0])
            if mode == "mcsolve" and not self._mc_fast_ok(problems[0]):
                if options.get("general_jumps"):
                    if mc_ntraj is not None and options.get("mc_ensemble"):
                        return [self._solve_general_jumps_ensemble(problems[0], mc_ntraj, options)]
                    return self._solve_general_jumps(problems, options, mc_ntraj)
                mode = "mesolve"
            if mode == "mcsolve":
                if mc_ntraj is not None:
                    if options.get("mc_ensemble"):
                        return [self._solve_mc_ensemble(problems[0], mc_ntraj, options)]
                    return [self._solve_mc_average(problems[0], mc_ntraj, options)]
            elif not self._fast_path_ok(problems[0]):
                return self._solve_general(problems, mode, options)
            tables = lower(problems)
        else:
            mode = self._solver_mode({"collapse_ops": [1] if tables.dissipator is not None else []})
            if mode == "mcsolve" and tables.collapse_local is None:
                mode = "mesolve"
        n_batch = tables.batch
        times = self._eval_times_array
        n = self._hamiltonian_data.n_qudits
        state_bytes = 16 * (4**n if mode == "mesolve" else 2**n) * n_batch
        on_device = mode == "mesolve" and state_bytes >= self._DEVICE_STATE_BYTES
        if on_device:
            self._check_snapshot_budget(len(times) - 1, state_bytes)
        with Engine(tables, mode=mode) as eng:
            init = np.asarray(self._initial_state)
            if mode == "mcsolve" and init.ndim == 2 and init.shape[0] == init.shape[1] and init.shape[0] > 1:
                raise NotImplementedError(
                    "Quantum-jump trajectories need a ket as initial state; use "
                    "solver=Solver.MESOLVER with a density matrix.")
            state = eng.new_state(init.reshape(1, -1))
            first = None if (on_device or raw) else state.cpu().numpy()  # (raw: nothing is wrapped, no host copy)
            first_dev = state.clone() if raw else None
            if mode == "mcsolve":
                snaps = eng.mc_solve(state, times, self._mc_seeds(n_batch, options), store=True,
                                     **self._engine_kwargs(options))
                self.last_mc_jumps = eng.mc_jumps()
                stats = eng.stats()
            else:
                ekw = self._engine_kwargs(options)
                plan = None if raw else self._window_plan(tables, mode, np.asarray(times, dtype=float), ekw)
                if plan is not None:
                    snaps, stats = self._solve_in_windows(eng, tables, state, np.asarray(times, dtype=float), ekw, plan)
                else:
                    snaps = eng.solve(state, times, store=True, **ekw)
                    stats = eng.stats()
            self.last_engine_stats = stats
            # large density matrices never cross PCIe as a whole: the results hold the device
            # tensors and reduce the diagonal (sampling weights, qutip_result.py:101-118) there
            if raw:
                occ = eng.torch.stack([eng.occupations(first_dev)]
                                      + [eng.occupations(snaps[i]) for i in range(len(times) - 1)]).cpu().numpy()
                return first_dev, snaps, occ
            # ... and the other snapshots stay in HBM until somebody reads them (evaluation_times="Full", the reference's
            # default, stores 3 101 states per sequence: 813 MB at 14 atoms); results.states hands out LazyState objects
            store = None if on_device else SnapshotStore(snaps)
            del state
        meas_errors = (
            {"epsilon": self.noise_model.p_false_pos, "epsilon_prime": self.noise_model.p_false_neg}
            if "SPAM" in self.noise_model.noise_types else None
        )
        qids = tuple(self.samples_obj.qubit_ids)
        basis_name = self.basis_name
        matching = self._meas_basis in basis_name
        t_unit = self._tot_duration * 1e-3
        shape = (tuple(first[0].shape) if first is not None and first[0].ndim == 2 else (2**n, 1))
        out = []
        for b in range(n_batch):
            results = []
            for i, t in enumerate(times):
                if on_device:
                    st: Any = (DeviceState(ket=np.asarray(self._initial_state).reshape(-1)) if i == 0
                               else DeviceState(tensor=snaps[i - 1][b]))
                elif i == 0:
                    st = QState(first[b])
                else:
                    st = LazyState(store, i - 1, b, shape)
                results.append(StateResult(qids, self._meas_basis, st, matching, evaluation_time=float(t / t_unit)))
            out.append(CoherentResults(results, n, basis_name, times, self._meas_basis, meas_errors))
        return out

    # density matrices from this size on stay on the GPU (13 atoms: 1 GiB per state)
    _DEVICE_STATE_BYTES = 1 << 30

    @staticmethod
    def _check_snapshot_budget(n_snapshots: int, state_bytes: int, what: str = "density matrix",
                               once_bytes: int = 0) -> None:
        """Refuse evaluation-time lists whose stored states cannot fit the device (the reference
        would fail the same way in host memory, after hours): the solver needs 4 work copies, the
        results one copy per evaluation time.  ``once_bytes``: what the run keeps on the device once, whatever the
        number of evaluation times (the targets and operators of an ensemble route)."""
        import torch

        free, total = torch.cuda.mem_get_info()
        need = (n_snapshots + 5) * state_bytes + once_bytes
        if need > 0.9 * free:
            raise MemoryError(
                f"Storing the state at {n_snapshots} evaluation times needs {need / 2**30:.0f} GiB of "
                f"device memory ({state_bytes / 2**30:.2f} GiB per {what}, {free / 2**30:.0f} GiB "
                "free): use evaluation_times='Minimal' or a short list of times instead of 'Full'."
            )

    @staticmethod
    def _fast_path_ok(problem: dict[str, Any]) -> bool:
        """2-level ground-rydberg / digital problems whose dissipator has only
        diagonal and double-flip entries run on the tuned matrix-free kernels;
        everything else takes the explicit-term general path."""
        from .terms import SUPPORTED_BASES, local_dissipator

        if problem["basis_name"] not in SUPPORTED_BASES or len(problem["eigenbasis"]) != 2:
            return False
        if problem.get("interaction_type") == "XY":
            return False
        S = local_dissipator(problem.get("collapse_ops", []), problem["eigenbasis"],
                             problem.get("depolarizing_pauli_2ds"))
        if S is not None:
            for r in range(4):
                for c in range(4):
                    if c not in (r, 3 - r) and S[r, c] != 0:
                        return False
        return True

    def _solve_mc_average(self, problem: dict[str, Any], ntraj: int,
                          options: dict[str, Any]) -> CoherentResults:
        """``qutip.mcsolve(..., ntraj=n_trajectories)`` of the deterministic run
        (simulation.py:726-727, 843): ``result.states`` is the trajectory-averaged
        density matrix at every evaluation time.  The trajectories run as GPU
        batches of kets; ``|psi><psi|`` is accumulated on the device."""
        from .engine import Engine
        from .terms import lower

        times = self._eval_times_array
        n = self._hamiltonian_data.n_qudits
        D = 2 ** n
        if (len(times) * D * D * 16) > (16 << 30):
            raise MemoryError(
                f"Averaged density matrices at {len(times)} evaluation times of a {n}-atom "
                "register do not fit; use fewer evaluation times.")
        init = np.asarray(self._initial_state)
        if init.ndim == 2 and init.shape[0] == init.shape[1] and init.shape[0] > 1:
            raise NotImplementedError(
                "Quantum-jump trajectories need a ket as initial state; use "
                "solver=Solver.MESOLVER with a density matrix.")
        chunk = int(max(1, min(ntraj, 1024, (2 << 30) // max(1, D * 16 * len(times)))))
        acc = None
        done = 0
        jumps = []
        while done < ntraj:
            b = min(chunk, ntraj - done)
            tables = lower([problem] * b)
            with Engine(tables, mode="mcsolve") as eng:
                torch = eng.torch
                if acc is None:
                    acc = torch.zeros((len(times), D, D), dtype=torch.complex128, device=eng.device)
                state = eng.new_state(init.reshape(1, -1))
                eng.outer_accumulate(state, acc[0])
                snaps = eng.mc_solve(state, times, self._mc_seeds(b, options), store=True,
                                     **self._engine_kwargs(options))
                for i in range(1, len(times)):
                    eng.outer_accumulate(snaps[i - 1], acc[i])
                jumps.append(eng.mc_jumps())
                self.last_engine_stats = eng.stats()
            done += b
        self.last_mc_jumps = np.concatenate(jumps)
        host = (acc / ntraj).cpu().numpy()
        meas_errors = (
            {"epsilon": self.noise_model.p_false_pos, "epsilon_prime": self.noise_model.p_false_neg}
            if "SPAM" in self.noise_model.noise_types else None
        )
        qids = tuple(self.samples_obj.qubit_ids)
        results = [
            StateResult(qids, self._meas_basis, QState(host[i]), self._meas_basis in self.basis_name,
                        evaluation_time=float(t / (self._tot_duration * 1e-3)))
            for i, t in enumerate(times)
        ]
        return CoherentResults(results, n, self.basis_name, times, self._meas_basis, meas_errors)

    def _solve_mc_ensemble(self, problem: dict[str, Any], ntraj: int,
                           options: dict[str, Any]) -> CoherentResults:
        """The deterministic quantum-jump run of :meth:`_solve_mc_average` (``run(mc_ensemble=True)``) without the
        averaged density matrices: the same chunks, seeds and kernels integrate the same trajectories, and what is
        linear in ``mean_b |psi_b><psi_b|`` is reduced from the kets - the diagonal by ``ensemble_diag``, the
        occupations, correlations and energy moments by ``observe_many`` of a noiseless batch-1 engine (the option
        ``mc_ensemble_observer`` hands one in; it is then left open) - and summed over the trajectories on the host.
        Memory is d^N per trajectory, never d^2N; the results hold :class:`EnsembleState` objects."""
        from .engine import Engine, ensemble_diag
        from .terms import lower

        times = self._eval_times_array
        n = self._hamiltonian_data.n_qudits
        D = 2 ** n
        init = np.asarray(self._initial_state)
        if init.ndim == 2 and init.shape[0] == init.shape[1] and init.shape[0] > 1:
            raise NotImplementedError(
                "Quantum-jump trajectories need a ket as initial state; use "
                "solver=Solver.MESOLVER with a density matrix.")
        chunk = int(max(1, min(ntraj, 1024, (2 << 30) // max(1, D * 16 * len(times)))))
        # per evaluation time: one row of the diagonals and the kets of one chunk (the solver's work copies are kets too)
        targets, operators = self._ensemble_observables(options)
        per_time, once = self._overlap_bytes(targets, operators, chunk)
        subsystems = self._ensemble_subsystems(options)
        # (one [dA, dA] accumulator per subsystem and evaluation time, and as much again for the partials of a split)
        per_time += sum(2 * 16 * 4 ** len(sub) for sub in subsystems)
        self._check_snapshot_budget(len(times) - 1, D * 8 + chunk * D * 16 + per_time,
                                    "evaluation time (the ensemble diagonal and one chunk of kets)", once)
        observer = options.get("mc_ensemble_observer")
        own_observer = observer is None
        if own_observer:
            noiseless = dict(problem)
            noiseless["collapse_ops"] = []
            observer = Engine.from_problems([noiseless], mode="sesolve")
        t_us = np.asarray(times, dtype=np.float64)
        sums = _EnsembleSums(len(times), n, n_targets=len(targets), operators=[operator_key(m) for m in operators])
        reduced_host: list[np.ndarray] = []
        add = sums.add
        try:
            torch = observer.torch
            overlaps = self._overlap_reducer(sums, targets, operators, observer.device)
            diag = torch.zeros((len(times), D), dtype=torch.float64, device=observer.device)
            first = observer.new_state(init.reshape(1, -1))[None]  # [1, 1, D]: every trajectory starts here
            ensemble_diag(first, diag[:1])
            diag[0] *= ntraj
            add(observer.observe_many(first, t_us[:1], energy=True), slice(0, 1), ntraj)
            overlaps(first, slice(0, 1), ntraj)
            reduced = []  # per subsystem: the trajectory sums [T, dA, dA] on the device
            if subsystems:
                from .engine import reduced_density

                for sub in subsystems:
                    acc = torch.zeros((len(times), 2 ** len(sub), 2 ** len(sub)), dtype=torch.complex128,
                                      device=observer.device)
                    reduced_density(first, sub, out=acc[:1])
                    acc[0] *= ntraj
                    reduced.append(acc)
            del first
            done = 0
            jumps = []
            while done < ntraj:
                b = min(chunk, ntraj - done)
                tables = lower([problem] * b)
                with Engine(tables, mode="mcsolve") as eng:
                    state = eng.new_state(init.reshape(1, -1))
                    snaps = eng.mc_solve(state, times, self._mc_seeds(b, options), store=True,
                                         **self._engine_kwargs(options))
                    ensemble_diag(snaps, diag[1:])
                    add(observer.observe_many(snaps, t_us[1:], energy=True), slice(1, None))
                    overlaps(snaps, slice(1, None))
                    for sub, acc in zip(subsystems, reduced):
                        reduced_density(snaps, sub, out=acc[1:])
                    jumps.append(eng.mc_jumps())
                    self.last_engine_stats = eng.stats()
                    del state, snaps
                done += b
            host = diag.cpu().numpy()
            reduced_host = [acc.cpu().numpy() for acc in reduced]
            del diag, reduced
        finally:
            if own_observer:
                observer.close()
        self.last_mc_jumps = np.concatenate(jumps)
        return self._ensemble_results(sums.states(host, ntraj, subsystems=subsystems, reduced_sums=reduced_host))

    def _ensemble_results(self, states: list[EnsembleState]) -> CoherentResults:
        """The results of an ensemble route: one ``StateResult`` per evaluation time around its ``EnsembleState``."""
        times = self._eval_times_array
        meas_errors = (
            {"epsilon": self.noise_model.p_false_pos, "epsilon_prime": self.noise_model.p_false_neg}
            if "SPAM" in self.noise_model.noise_types else None
        )
        qids = tuple(self.samples_obj.qubit_ids)
        results = [
            StateResult(qids, self._meas_basis, st, self._meas_basis in self.basis_name,
                        evaluation_time=float(t / (self._tot_duration * 1e-3)))
            for st, t in zip(states, times)
        ]
        return CoherentResults(results, self._hamiltonian_data.n_qudits, self.basis_name, times, self._meas_basis,
                               meas_errors)

    def _solve_general_jumps_ensemble(self, problem: dict[str, Any], ntraj: int,
                                      options: dict[str, Any]) -> CoherentResults:
        """The deterministic run of :meth:`_solve_general_jumps` (``run(general_jumps=True, mc_ensemble=True)``) without
        the averaged density matrices, as :meth:`_solve_mc_ensemble` is to :meth:`_solve_mc_average`: the same tables,
        chunks, seeds and ``GeneralEngine.mc_solve`` calls integrate the same trajectories bit for bit; the diagonal
        is reduced from the kets by ``ensemble_diag``, the occupations and correlations of every local state in
        ``mc_ensemble_digits`` and the energy moments (with the first digit) by ``GeneralEngine.observe_many`` of a
        noiseless batch-1 ket engine lowered matrix-free (``mc_ensemble_observer`` hands one in; it is left open).
        The energy moments need the padded-table application of that engine (``apply_path()`` ``fused`` /
        ``fused_lds``); a problem of more than 96 terms is lowered to CSR terms instead, and ``energy`` / ``energy2``
        of its results are ``nan`` while the diagonal and the pair sums are served as usual."""
        from .engine import GeneralEngine, ensemble_diag
        from .general import lower_general
        from .results import _ONE_STATE

        times = self._eval_times_array
        n = self._hamiltonian_data.n_qudits
        eigenbasis = list(problem["eigenbasis"])
        digits = options.get("mc_ensemble_digits")
        if digits is None:
            digits = [eigenbasis.index(_ONE_STATE[self._meas_basis])]
        digits = list(dict.fromkeys(int(v) for v in digits))  # distinct, in the order asked for
        if not digits or any(not 0 <= v < len(eigenbasis) for v in digits):
            raise ValueError(f"mc_ensemble_digits must be local-state indices in [0, {len(eigenbasis)}) "
                             f"({tuple(eigenbasis)}), got {digits}")
        init = np.asarray(self._initial_state)
        if init.ndim == 2 and init.shape[0] == init.shape[1] and init.shape[0] > 1:
            raise NotImplementedError(
                "Quantum-jump trajectories need a ket as initial state; use "
                "solver=Solver.MESOLVER with a density matrix.")
        ket = init.reshape(-1)
        kw = self._engine_kwargs(options, general=True)
        tables, cops = lower_general(problem, mesolve=False, with_collapse=True)
        D = tables.dim
        chunk = int(max(1, min(ntraj, 1024, (2 << 30) // max(1, D * 16 * len(times)))))
        # per evaluation time: one row of the diagonals and the kets of one chunk (the solver's work copies are kets too)
        targets, operators = self._ensemble_observables(options)
        per_time, once = self._overlap_bytes(targets, operators, chunk)
        self._check_snapshot_budget(len(times) - 1, D * 8 + chunk * D * 16 + per_time,
                                    "evaluation time (the ensemble diagonal and one chunk of kets)", once)
        observer = options.get("mc_ensemble_observer")
        own_observer = observer is None
        if own_observer:
            noiseless = dict(problem)
            noiseless["collapse_ops"] = []
            observer = GeneralEngine(lower_general(noiseless, mesolve=False, matrix_free=True))
        t_us = np.asarray(times, dtype=np.float64)
        sums = _EnsembleSums(len(times), n, digits, n_targets=len(targets), operators=[operator_key(m) for m in operators])
        try:
            with_energy = observer.apply_path() in ("fused", "fused_lds")
            overlaps = self._overlap_reducer(sums, targets, operators, observer.device)

            def observe(kets: Any, t: np.ndarray, at: slice, weight: int = 1) -> None:
                for k, digit in enumerate(digits):  # (only the first call carries the energy moments)
                    sums.add(observer.observe_many(kets, t, one=digit, energy=with_energy and k == 0), at, weight, digit)

            torch = observer.torch
            diag = torch.zeros((len(times), D), dtype=torch.float64, device=observer.device)
            first = observer.new_state(ket)[None]  # [1, 1, D]: every trajectory starts here
            ensemble_diag(first, diag[:1])
            diag[0] *= ntraj
            observe(first, t_us[:1], slice(0, 1), ntraj)
            overlaps(first, slice(0, 1), ntraj)
            del first
            done = 0
            jumps = []
            while done < ntraj:
                b = min(chunk, ntraj - done)
                with GeneralEngine(tables, batch=b) as eng:
                    eng.set_collapse(cops)
                    state = eng.new_state(ket)
                    snaps = eng.mc_solve(state, times, self._mc_seeds(b, options), **kw)
                    ensemble_diag(snaps, diag[1:])
                    observe(snaps, t_us[1:], slice(1, None))
                    overlaps(snaps, slice(1, None))
                    jumps.append(eng.mc_jumps())
                    self.last_engine_stats = eng.stats()
                    del state, snaps
                done += b
            host = diag.cpu().numpy()
            del diag
        finally:
            if own_observer:
                observer.close()
        self.last_mc_jumps = np.concatenate(jumps)
        return self._ensemble_results(sums.states(host, ntraj, with_energy=with_energy, by_digit=True))

    def _solve_general(self, problems: list[dict[str, Any]], mode: str,
                       options: dict[str, Any]) -> list[CoherentResults]:
        from .engine import GeneralEngine
        from .general import lower_general

        times = self._eval_times_array
        meas_errors = (
            {"epsilon": self.noise_model.p_false_pos, "epsilon_prime": self.noise_model.p_false_neg}
            if "SPAM" in self.noise_model.noise_types else None
        )
        qids = tuple(self.samples_obj.qubit_ids)
        n = self._hamiltonian_data.n_qudits
        out = []
        kw = self._engine_kwargs(options, general=True)
        # ``general_device_snapshots`` (sesolve kets): the solved tensor stays in HBM behind a SnapshotStore, one per
        # trajectory, and the results hold LazyState objects - what the 2-level path always does
        # ``general_density_snapshots`` (mesolve matrices): the same, every snapshot viewed as a [D, D] matrix
        keep_dm = bool(options.get("general_density_snapshots")) and mode == "mesolve"
        keep = (bool(options.get("general_device_snapshots")) and mode == "sesolve") or keep_dm
        solved: list[tuple[np.ndarray, Any]] = []
        engines = [GeneralEngine(lower_general(prob, mesolve=(mode == "mesolve"))) for prob in problems]
        try:
            if keep:
                # every trajectory's snapshot tensor is on the device at once (the stores are built after the last
                # solve), next to each engine's work vectors: the budget counts the kets of ALL trajectories per time
                self._check_snapshot_budget(len(times) - 1, 16 * sum(eng.dim for eng in engines),
                                            "evaluation time (the density matrices of all trajectories)" if keep_dm
                                            else "evaluation time (the kets of all trajectories)")
            states = [eng.new_state(np.asarray(self._initial_state).reshape(-1)) for eng in engines]
            firsts = [st.cpu().numpy()[0] for st in states]
            if len(engines) > 1 and all(eng.dim <= 4096 for eng in engines) and np.all(np.diff(times) > 0):
                # the trajectories of a multi-level / XY run: one launch, one workgroup per trajectory
                snaps = GeneralEngine.solve_many(engines, states, times, **kw)
                solved = [(f, s if keep else s.cpu().numpy()) for f, s in zip(firsts, snaps)]
                self.last_engine_stats = engines[0].stats()
            else:
                for eng, st, f in zip(engines, states, firsts):
                    snap = eng.solve(st, times, **kw)
                    solved.append((f, snap if keep else snap.cpu().numpy()))
                    self.last_engine_stats = eng.stats()
        finally:
            for eng in engines:
                eng.close()
        for prob, (first, host) in zip(problems, solved):
            D = len(prob["eigenbasis"]) ** n
            if keep_dm:  # [T - 1, 1, D * D] as solved: a view, nothing moves
                host = host.reshape(host.shape[0], 1, D, D)
            store = SnapshotStore(host) if keep else None
            results = []
            for i, t in enumerate(times):
                st: Any
                if keep:
                    if i == 0:
                        st = QState(first.reshape(D, D) if keep_dm else first)
                    else:
                        st = LazyState(store, i - 1, 0, (D, D) if keep_dm else (D, 1))
                else:
                    st = first if i == 0 else host[i - 1][0]
                    if mode == "mesolve":
                        st = st.reshape(D, D)
                    st = QState(st)
                results.append(
                    StateResult(qids, self._meas_basis, st,
                                self._meas_basis in self.basis_name,
                                evaluation_time=float(t / (self._tot_duration * 1e-3))))
            out.append(CoherentResults(results, n, self.basis_name, times, self._meas_basis,
                                       meas_errors))
        return out

    def _solve_general_jumps(self, problems: list[dict[str, Any]], options: dict[str, Any],
                             mc_ntraj: int | None) -> list[CoherentResults]:
        """``qutip.mcsolve`` for the problems the tuned jump kernels do not take (multi-level bases, XY mode,
        a non-diagonal ``sum C^dag C``), as quantum-jump trajectories on the general path (``run(...,
        general_jumps=True)``).  ``mc_ntraj=None``: one trajectory per problem (the noisy runs), kets as results;
        else the deterministic run: ``mc_ntraj`` trajectories of ``problems[0]`` averaged into density matrices
        like :meth:`_solve_mc_average`."""
        from .engine import GeneralEngine
        from .general import lower_general

        times = self._eval_times_array
        n = self._hamiltonian_data.n_qudits
        init = np.asarray(self._initial_state)
        if init.ndim == 2 and init.shape[0] == init.shape[1] and init.shape[0] > 1:
            raise NotImplementedError(
                "Quantum-jump trajectories need a ket as initial state; use "
                "solver=Solver.MESOLVER with a density matrix.")
        ket = init.reshape(-1)
        kw = self._engine_kwargs(options, general=True)
        meas_errors = (
            {"epsilon": self.noise_model.p_false_pos, "epsilon_prime": self.noise_model.p_false_neg}
            if "SPAM" in self.noise_model.noise_types else None
        )
        qids = tuple(self.samples_obj.qubit_ids)
        t_unit = self._tot_duration * 1e-3

        def wrap(states: list[np.ndarray]) -> CoherentResults:
            results = [StateResult(qids, self._meas_basis, QState(st), self._meas_basis in self.basis_name,
                                   evaluation_time=float(t / t_unit)) for st, t in zip(states, times)]
            return CoherentResults(results, n, self.basis_name, times, self._meas_basis, meas_errors)

        if mc_ntraj is not None:
            tables, cops = lower_general(problems[0], mesolve=False, with_collapse=True)
            D = tables.dim
            if (len(times) * D * D * 16) > (16 << 30):
                raise MemoryError(
                    f"Averaged density matrices at {len(times)} evaluation times of a {n}-atom "
                    "register do not fit; use fewer evaluation times.")
            from .engine import outer_accumulate

            chunk = int(max(1, min(mc_ntraj, 1024, (2 << 30) // max(1, D * 16 * len(times)))))
            acc = None
            done = 0
            jumps = []
            while done < mc_ntraj:
                b = min(chunk, mc_ntraj - done)
                with GeneralEngine(tables, batch=b) as eng:
                    eng.set_collapse(cops)
                    torch = eng.torch
                    if acc is None:
                        acc = torch.zeros((len(times), D, D), dtype=torch.complex128, device=eng.device)
                    state = eng.new_state(ket)
                    outer_accumulate(state, acc[0])
                    snaps = eng.mc_solve(state, times, self._mc_seeds(b, options), **kw)
                    for i in range(1, len(times)):
                        outer_accumulate(snaps[i - 1], acc[i])
                    jumps.append(eng.mc_jumps())
                    self.last_engine_stats = eng.stats()
                done += b
            self.last_mc_jumps = np.concatenate(jumps)
            return [wrap(list((acc / mc_ntraj).cpu().numpy()))]

        lowered = [lower_general(prob, mesolve=False, with_collapse=True) for prob in problems]
        seeds = self._mc_seeds(len(problems), options)
        engines = [GeneralEngine(tables) for tables, _ in lowered]
        try:
            for eng, (_, cops) in zip(engines, lowered):
                eng.set_collapse(cops)
            states = [eng.new_state(ket) for eng in engines]
            first = states[0].cpu().numpy()[0]
            if len(engines) > 1 and all(eng.dim <= 4096 for eng in engines) and np.all(np.diff(times) > 0):
                snaps = GeneralEngine.mc_solve_many(engines, states, times, seeds, **kw)
            else:
                snaps = [eng.mc_solve(st, times, seeds[i:i + 1], **kw)
                         for i, (eng, st) in enumerate(zip(engines, states))]
            self.last_mc_jumps = np.concatenate([eng.mc_jumps() for eng in engines])
            self.last_engine_stats = engines[0].stats()
            hosts = [s.cpu().numpy() for s in snaps]
        finally:
            for eng in engines:
                eng.close()
        return [wrap([first] + [h[i][0] for i in range(len(times) - 1)]) for h in hosts]

    def run(self, progress_bar: bool = False, print_progress: bool = False,
            **options: Any) -> SimulationResults:
        """simulation.py:800-883.  ``options`` accepts QuTiP's ``max_step`` (an
        upper bound on the step, us) plus the engine's ``tol``,
        ``taylor_order``, ``magnus_tol``; QuTiP-only keys are ignored.

        ``general_jumps=True``: problems that take ``qutip.mcsolve`` but not the tuned 2-level jump kernels
        (3- / 4-level bases, XY mode, collapse operators whose ``sum C^dag C`` is not diagonal) run as
        quantum-jump trajectories on the general path - kets of d^N amplitudes, so registers beyond the
        master equation's 2^26-entry Liouvillian (XY up to 26 atoms, 3 levels up to 16) - instead of the
        default master-equation fallback.  Seeds follow ``seeds=`` exactly as on the 2-level path.

        ``general_device_snapshots=True``: the kets of a multi-level / XY run without collapse operators stay on the
        GPU (one ``SnapshotStore`` per trajectory) and ``results.states`` holds ``LazyState`` objects that cross PCIe
        when they are read, as the states of a 2-level run do; by default they are host ``QState`` objects.

        ``general_density_snapshots=True``: the same for the density matrices of a multi-level / XY master-equation run
        (collapse operators, ``eff_noise``): the solved ``[T - 1, 1, D, D]`` tensor of every trajectory stays on the GPU
        behind its own ``SnapshotStore`` (16 D^2 bytes per trajectory and evaluation time, checked against the snapshot
        budget for all trajectories together before the solve) and the results hold ``LazyState`` matrices; the
        initial state stays a host ``QState``.  A run without collapse operators ignores it, as a master-equation run
        ignores ``general_device_snapshots``.

        ``mc_ensemble=True``: the deterministic-noise quantum-jump run on the tuned 2-level jump kernels
        (``Solver.MCSOLVER`` / ``n_trajectories`` on one Hamiltonian) keeps d^N numbers per trajectory to the end: the
        trajectory-averaged density matrices are not formed, so the evaluation-time list is no longer capped by
        16 GiB of ``[D, D]`` accumulators (3 times at 14 atoms).  The same trajectories run on the same kernels with
        the same ``seeds=``; the results hold ``EnsembleState`` objects - the diagonal of the averaged state
        (sampling, ``sampling_dist``, the SPAM flips and ``expect`` of diagonal operators work unchanged) and the
        trajectory means ``occupation``, ``correlation``, ``energy``, ``energy2``, ``norm2`` with
        ``occupation_stderr``, equal to the values of the averaged matrix within rounding.  ``full()``, ``overlap``
        and ``expect`` of other operators raise ``NotImplementedError`` (but see ``mc_ensemble_operators``).  Every
        other run ignores the option (but see ``general_jumps`` with it, below).
        ``mc_ensemble_observer``: a noiseless batch-1 sesolve ``Engine`` whose H(t) the energy moments use (left
        open); by default one is built from the run's problem without its collapse operators.
        ``mc_ensemble_targets``: F kets, ``[F, D]`` or a list of ``[D]`` / ``[D, 1]`` arrays (D = d^N, the run's
        eigenbasis order): ``EnsembleState.fidelity`` [F] is the fidelity ``<phi|rho|phi>`` of the averaged state with
        each, the trajectory mean of ``|<phi|psi_b>|^2`` (one ``overlap_many`` call per chunk of trajectories), and
        ``fidelity_stderr`` its Monte-Carlo error.  A matrix (a mixed target) raises ``ValueError``: it needs the
        default route.
        ``mc_ensemble_operators``: K operators of shape ``(D, D)`` - arrays, SciPy sparse matrices or ``qutip.Qobj``,
        as ``results.expect`` takes them: ``EnsembleState.expectation`` [K] is ``Tr(O rho)``, the trajectory mean of
        ``<psi_b|O|psi_b>`` (one ``expect_sparse`` call per operator and chunk), with ``expectation_stderr``;
        ``results.expect`` then serves these operators - recognised by their shape and stored non-zeros - next to
        the diagonal ones.  Neither value is divided by ``norm2``.  Both options are used by the two ensemble routes
        alone and ignored by every other run; a wrong shape or a non-numeric entry raises ``ValueError`` before
        anything is solved.
        ``mc_ensemble_subsystems``: site tuples such as ``[(0, 1), (3, 4, 5)]`` (positions in the register's qubit ids,
        at most 6 each): the reduced density matrix ``mean_b Tr_rest |psi_b><psi_b|`` of each is reduced from the kets
        (one ``reduced_density`` call per subsystem and chunk of trajectories into a ``[T, dA, dA]`` device
        accumulator, read once at the end) - every expectation value of every operator supported on those atoms.
        ``EnsembleState.ptrace``, ``results.reduced_states`` and ``results.entanglement_entropy`` serve these
        subsystems and refuse any other.  Not divided by ``norm2``.  Used by the two-level ensemble route alone; an entry
        that is no tuple of distinct sites in range, or one of more than 6 sites, raises ``ValueError`` before anything
        is solved.

        ``general_jumps=True`` with ``mc_ensemble=True``: the same for the deterministic-noise run of the general
        path (multi-level bases, XY mode, a non-diagonal ``sum C^dag C``): the trajectories of ``general_jumps=True``
        alone, bit for bit, reported as ``EnsembleState`` objects instead of ``[D, D]`` averages - 14 and more XY
        atoms or 9 and more three-level atoms at any list of evaluation times.  ``mc_ensemble_digits``: the local
        states (indices into the eigenbasis) whose occupations and correlations are kept, by default the one-state of
        the measurement basis; ``EnsembleState.by_digit`` holds them all, ``occupation`` / ``correlation`` /
        ``occupation_stderr`` those of the first.  An index outside ``[0, d)`` raises ``ValueError``.
        ``mc_ensemble_observer`` is then a noiseless batch-1 ket ``GeneralEngine`` lowered matrix-free.  A problem of
        more than 96 Hamiltonian terms has no padded-table application: ``energy`` and ``energy2`` of its results
        are ``nan``, the diagonal and the pair sums are served as usual."""
        warnings.warn(
            "QutipEmulator is deprecated as of pulser 1.9. Please use QutipBackendV2 instead.",
            DeprecationWarning,
            stacklevel=2,
        )
        self._validate_options(options)
        if not has_stochastic_noise(self.noise_model):
            if print_progress:
                print("Emulating Trajectory 1/1")
            return self._solve_batch([self._current_problem], progress_bar, options,
                                     mc_ntraj=self.n_trajectories or 1)[0]

        sharded = self._distributed()
        if sharded is not None:
            # one process per GPU: trajectories shard over the ranks, one all-reduce of the
            # histograms; every rank returns the same NoisyResults (pulser_amd/distributed.py)
            from .distributed import run_ensemble

            ens = run_ensemble(self, dist=sharded, options=options, options_validated=True)
            qids = tuple(self.samples_obj.qubit_ids)
            results = [
                SampledResult(qids, self._meas_basis, ens["counters"][ind],
                              evaluation_time=float(t / (self._tot_duration * 1e-3)))
                for ind, t in enumerate(self._eval_times_array)
            ]
            return NoisyResults(results, self._hamiltonian_data.n_qudits, self.basis_name,
                                self._eval_times_array, int(ens["n_measures"]))

        total_count = np.array([Counter() for _ in self._eval_times_array])
        for res, reps in self._noisy_runs(progress_bar, print_progress, **options):
            total_count += np.array(
                [
                    res.sample_state(t, n_samples=self.noise_model.samples_per_run * reps)
                    for t in self._eval_times_array
                ]
            )
        n_measures = cast(int, self.n_trajectories) * self.noise_model.samples_per_run
        qids = tuple(self.samples_obj.qubit_ids)
        results = [
            SampledResult(qids, self._meas_basis, total_count[ind],
                          evaluation_time=float(t / (self._tot_duration * 1e-3)))
            for ind, t in enumerate(self._eval_times_array)
        ]
        return NoisyResults(results, self._hamiltonian_data.n_qudits, self.basis_name,
                            self._eval_times_array, n_measures)

    @staticmethod
    def _distributed() -> Any:
        """``torch.distributed`` when this process is one of several ranks, else None."""
        import sys

        td = sys.modules.get("torch.distributed")
        if td is None or not td.is_available() or not td.is_initialized() or td.get_world_size() < 2:
            return None
        from .distributed import sharding_enabled

        # an explicit opt-in: a process group may exist for reasons of the caller's own
        return td if sharding_enabled() else None

    def _refresh_trajectories_if_used(self) -> None:
        """Fresh noise-trajectory draws on every run after the first (simulation.py:892-900)."""
        if self._noise_trajectories_used:
            nm = self._hamiltonian_data.noise_model
            self._hamiltonian_data = HamiltonianData(
                self.samples_obj, nm, self._get_n_trajectories(nm, check_value=True))
            self._problems_cache = None

    def _noisy_runs(self, progress_bar: Any = False, print_progress: bool = False,
                    batch: int | None = None, only: tuple[int, int] | None = None, **options: Any
                    ) -> Iterator[tuple[CoherentResults | None, int]]:
        """simulation.py:885-915; trajectories are solved in GPU batches but
        yielded (and therefore sampled) in the reference's serial order.  ``only = (lo, hi)``
        (sharded runs): trajectories outside the block are yielded as ``(None, reps)`` unsolved."""
        n_trajectories = self.n_trajectories
        self._refresh_trajectories_if_used()
        self._noise_trajectories_used = True
        hd = self._hamiltonian_data
        trajs = hd.noise_trajectories
        if self._problems_cache is not None:  # an explicit (possibly trimmed) list wins
            trajs = trajs[: len(self._problems_cache)]
        n_eval = len(self._eval_times_array)
        is_me = len(self._current_problem["collapse_ops"]) > 0
        dim_bytes = 16 * (2 ** hd.n_qudits) ** (2 if is_me else 1)
        if batch is None:  # keep the snapshot tensor under ~8 GB
            batch = int(max(1, min(256, (8 << 30) // max(1, dim_bytes * n_eval))))
        traj_nb = 0
        if only is not None:
            lo, hi = only
            for tr in trajs[:lo]:
                yield None, tr.reps
            for start in range(lo, hi, batch):
                chunk = trajs[start:min(hi, start + batch)]
                if self._fast_path_ok(self._current_problem):
                    solved = self._solve_batch([], progress_bar, options,
                                               tables=hd.device_tables(chunk, self._sampling_rate))
                else:
                    solved = self._solve_batch([hd.problem(t, self._sampling_rate) for t in chunk],
                                               progress_bar, options)
                for tr, res in zip(chunk, solved):
                    yield res, tr.reps
            for tr in trajs[hi:]:
                yield None, tr.reps
            return
        for start in range(0, len(trajs), batch):
            chunk = trajs[start:start + batch]
            if self._fast_path_ok(self._current_problem):
                tables = hd.device_tables(chunk, self._sampling_rate)
                solved = self._solve_batch([], progress_bar, options, tables=tables)
            else:
                solved = self._solve_batch([hd.problem(t, self._sampling_rate) for t in chunk],
                                           progress_bar, options)
            for tr, res in zip(chunk, solved):
                reps = tr.reps
                if print_progress:
                    if reps == 1:
                        print(f"Emulating Trajectory {traj_nb+1}/{n_trajectories}")
                    else:
                        print("Emulating Trajectories "
                              f"[{traj_nb+1} - {traj_nb+reps}]/{n_trajectories}")
                traj_nb += reps
                yield res, reps

    @classmethod
    def from_sequence(cls, sequence: Any, sampling_rate: float = 1.0,
                      config: Optional[SimConfig] = None,
                      evaluation_times: Union[float, str, Any] = "Full",
                      with_modulation: bool = False, noise_model: Any = None,
                      solver: Solver = Solver.DEFAULT,
                      n_trajectories: int | None = None) -> "QutipEmulator":
        """simulation.py:955-1051 - needs ``pulser`` for the sampler."""
        if not (hasattr(sequence, "is_parametrized") and hasattr(sequence, "_schedule")):
            raise TypeError("The provided sequence has to be a valid pulser.Sequence instance.")
        if sequence.is_parametrized() or sequence.is_register_mappable():
            raise ValueError(
                "The provided sequence needs to be built to be simulated. Call"
                " `Sequence.build()` with the necessary parameters."
            )
        if not sequence._schedule:
            raise ValueError("The provided sequence has no declared channels.")
        if all(sequence._schedule[x][-1].tf == 0 for x in sequence.declared_channels):
            raise ValueError("No instructions given for the channels in the sequence.")
        if with_modulation and sequence._slm_mask_targets:
            raise NotImplementedError(
                "Simulation of sequences combining an SLM mask and output "
                "modulation is not supported."
            )
        from pulser.sampler import sampler  # user-side dependency

        samples = sampler.sample(
            sequence, modulation=with_modulation,
            extended_duration=sequence.get_duration(include_fall_time=with_modulation),
        )
        return cls(samples, sequence.register, sequence.device, sampling_rate, config,
                   evaluation_times, noise_model=noise_model, solver=solver,
                   n_trajectories=n_trajectories)
