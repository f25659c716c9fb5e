"""
qingdai_amd/driver.py -- drop-in for the reference driver `scripts/run_simulation.py:main()`
(run_simulation.py:1161-2523) with the per-timestep loop resident on the MI355X.

Kept from the reference driver: the QD_* environment surface of the path (plus QD_N_LAT / QD_N_LON,
which the reference only honours in its facade and topography generator -- SURVEY.md section 0.1),
procedural seed-42 or NetCDF topography, slab-ocean heat capacities, restart load/save
(QD_RESTART_IN / QD_RESTART_OUT, variables u v h T_s cloud_cover q h_ice uo vo eta Ts W_land S_snow
C_snow land_mask as f4 + scalar t_seconds, run_simulation.py:63-183), SIGINT/SIGTERM/atexit autosave
(run_simulation.py:1689-1706, exit codes 130/143), QD_SIM_DAYS / QD_TOTAL_YEARS / QD_DT_SECONDS,
QD_USE_OCEAN, the QD_USE_OO(_STRICT) short-circuit, periodic diagnostics.
Ecology (QD_ECO_ENABLE, default on like the reference): the per-step part -- EcologyAdapter.step_subdaily, the alpha blend
into the base albedo, IndividualPool.try_substep -- runs inside the resident loop (qingdai_amd/ecology.py, qd_eco_*); the
DAILY population dynamics are host code outside this package, reached through `Simulation(daily_hook=...)`, which is called
where the reference calls eco.step_daily (run_simulation.py:1786-1864).  Without a hook the LAI stays at its initial value.
Phytoplankton (QD_PHYTO_ENABLE and QD_PHYTO_ADVECTION, default on like the reference, needs the ocean): the per-step transport of
the tracers by the ocean currents (phyto.advect_diffuse, run_simulation.py:2254-2258) runs inside the resident loop on resident
tracers (qingdai_amd/phyto.py PhytoTracers, qd_phyto_*); data/plankton.nc carries C_phyto_s through autosave / startup load.
River routing (P014; QD_HYDRO_ENABLE default 1, QD_HYDRO_NETCDF default data/hydrology.nc, QD_HYDRO_DT_HOURS default 6,
QD_HYDRO_DIAG default 1, run_simulation.py:1294-1321): the network file is planned once on the host (qingdai_amd/routing.py), the
accumulation and the events run inside the resident loop after the snow commit + land bucket (qd_step_n bit7), and each chunk's
[HydroRouting] event lines are printed after it from the device event log.  A missing network file is generated on the device
(qingdai_amd/hydronet.py, the reference's run_simulation.py:1063-1127 bit for bit) when QD_HYDRO_AUTOGEN=1 -- the reference's
behaviour; by default (QD_HYDRO_AUTOGEN=0) the run goes on WITHOUT routing, with the reference's message.  The routing buffer is
not part of the restart files (as in the reference).
Phytoplankton daily step (P017; QD_PHYTO_DAILY=1, default 0, with QD_PHYTO_ENABLE=1): PhytoManager.step_daily runs inside the
resident loop on the steps its firing clock names (qd_step_n bit8, at the top of the step; qingdai_amd/phyto.py PhytoDaily), the
ocean-colour albedo overrides the ocean base albedo from the first daily step on (QD_PHYTO_ALBEDO_COUPLE, default 1), each chunk's
[PhytoDiag] lines are printed after it from the device log, and data/plankton.nc is written and read with the reference's
variable set.  The tracers exist then even without the ocean (the transport still needs it).
Daily vegetation dynamics (QD_ECO_DAILY=1, default 0, with QD_ECO_ENABLE=1 and no daily_hook): PopulationManager.step_daily --
growth, senescence, layered allocation, per-species spread, seed bank, age -- runs inside the resident loop on the steps the
reference's day accumulator names (qd_step_n bit9, at the top of the step; qingdai_amd/ecology.py PopulationDaily), spans are no
longer cut at day boundaries, and each chunk's `[Ecology] daily:` lines are printed after it from the device log (QD_ECO_DIAG=1).
QD_ECO_MUT_RATE > 0 is refused with it unless QD_ECO_SPECIATION=1 is set.
Speciation (QD_ECO_SPECIATION=1, default 0; needs QD_ECO_DAILY=1 and no daily_hook; adapter.py:437-515, run_simulation.py:1847-1861):
behind every daily firing the reference draws rand() against QD_ECO_MUT_RATE and, on a hit below QD_ECO_SPECIES_MAX, picks a parent
by species weight, splits QD_ECO_MUT_EPS of its LAI into a new species, mutates its genes and rebuilds the reflectance table --
inside the step, before the rest of it.  Here `speciation_due` walks the firings of the steps ahead, draws each firing's rand() once
(kept by firing number, in firing order, no further than the first hit), and a chunk ends with the step BEFORE a hit's step; that
step's firings then run through the lane's class seam (qd_eco_daily_step on the resident soil water), each followed by
ecology.Speciation.event -- the split on the resident stack (qd_eco_daily_speciate), Gene.mutated, the table, the reference's
`[Ecology] mutation:` lines -- and, under QD_ECO_BANDS_COUPLE=1, the banded alpha; the step itself runs with those firings struck
out of the lane's schedule.  QD_ECO_GENES_EXPORT=1 writes <QD_OUTPUT_DIR>/genes_day_*.json for every firing after its chunk (weights
and genes are constant within one), as often as the reference prints its line.  Refused at start-up: QD_ECO_INDIV_DAILY=1 (the pool
was sampled for the run's species), QD_ECO_MUT_EPS <= 0 (the reference then truncates its gene table), QD_ECO_SPECIES_MAX > 64.
Saving and resuming the vegetation state (QD_ECO_PERSIST, default 0; run_simulation.py:248-305, 1464-1488, 1566-1590,
pygcm/ecology/adapter.py:284-426, 574-777): at 1 every autosave writes data/ecology.nc (QD_ECO_AUTOSAVE_PATH when that ends in .nc;
the reference's variable set, a time-stamped copy, QD_ECO_AUTOSAVE_KEEP of them kept) behind data/atmosphere.nc and data/genes.json
behind that, and start-up -- behind the atmosphere / ocean block, gated by QD_AUTOSAVE_LOAD alone, after the individuals were
sampled -- reads genes.json (QD_ECO_GENES_JSON_PATH) and then the ecology file (QD_ECO_AUTOSAVE_PATH, QD_ECO_ON_MISMATCH) with the
reference's [Ecology] lines.  The load rebuilds the LAI stack from the file's one plane on the device (qd_eco_state_restore) in the
reference's arithmetic; at 2 the file also carries qd_* variables with which the ecology lanes resume bit for bit.
Daily step of the individuals (QD_ECO_INDIV_DAILY=1, default 0; needs QD_ECO_DAILY=1, QD_ECO_ENABLE=1, a population, individuals
and no daily_hook, else refused at start-up): IndividualPool.step_daily (individuals.py:193-361, run_simulation.py:1818-1835) runs
on the device directly behind every firing of the daily vegetation step, on the same soil index (qingdai_amd/ecology.py
IndividualDaily) -- species shares and LAI of the sampled cells, recruits, seed bank, species_weights (which the next day's
germination, the banded albedo and the true-colour frame then use), the individuals' buffers -- and each chunk's `[EcoIndiv] daily
applied` lines are printed after it from the device log (QD_ECO_DIAG=1).  At 0 the note that the step is not run stays.
Diversity diagnostics (QD_ECO_DIVERSITY_ENABLE=1, default 0; QD_ECO_DIVERSITY_EVERY_DAYS, default 10; run_simulation.py:2406-2414,
pygcm/ecology/diversity.py): on the reference's clock -- the step whose start time t_i satisfies t_i / day >= next fires at its end
and sets next = t_i / day + every, so the first step always fires -- the alpha map, the local Bray-Curtis map and the Whittaker
summary are computed on the device from the LAI stack (the resident one under QD_ECO_DAILY=1; PopulationCanopy.diversity), a chunk
ends with the firing step, and the reference's files go to <QD_OUTPUT_DIR, default output>/ecology/ named by t_i / day:
diversity_summary_day_*.txt and community_day_*.npz as the reference writes them, diversity_maps_day_*.npz (alpha_map, bc_local)
in place of its two PNG maps.  QD_ECO_DIAG=1 prints one [Diversity] line per firing.
True-colour frames (QD_TRUECOLOR=1, default 0; QD_PLOT_EVERY_DAYS, default 10; plot_true_color, run_simulation.py:539-778,
2426-2429): on the reference's plot clock -- the step with run-local index i % plot_interval_steps == 0 fires at its end, labelled
by its start time t_i / day -- the frame is composed on the device from the resident state (qingdai_amd/truecolor.py,
qd_truecolor_*), a chunk ends with the firing step, and each firing writes <QD_OUTPUT_DIR, default output>/true_color_day_*.png
(n_lat x n_lon pixels, no axes) and prints the reference's [TrueColor] sea-ice line.
Procedural planet on the device (QD_TOPO_DEVICE=1, default 0): without a QD_TOPO_NC file the land mask comes from
qingdai_amd/topogen.py (qd_topogen_build) with the reference driver's settings -- seed 42, land fraction 0.29, no overrides, no
elevation map -- instead of the host recipe of qingdai_amd/topography.py; base properties and the [Topo] line are the same.  The
device's elevation agrees with the host's to about 1e-11 m, so the two masks can differ only in a cell whose elevation lies that
close to sea level; the default stays 0 for that reason.
Periodic budget lines (QD_BUDGET_DIAG=1, default 0; run_simulation.py:2148-2188, 2263-2287, 2349-2398, pygcm/ocean.py:446-516): the
reference's [EnergyDiag], [OceanDiag], [HumidityDiag], [WaterDiag] and [HydroRoutingDiag] on steps with run-local index i % 200 == 0
and its ocean's [OceanE] on the ocean's own step count % QD_OCEAN_DIAG_EVERY, selected by the reference's QD_ENERGY_DIAG,
QD_OCEAN_DIAG, QD_OCEAN_ENERGY_DIAG, QD_HUMIDITY_DIAG, QD_WATER_DIAG (all default 1) and QD_OCEAN_POLAR_LAT.  A fourth span lane
(qingdai_amd/budget_diag.py, qd_budget_diag_*): chunks are NOT cut at firing steps; the device reduces at the reference's positions
inside the step and each chunk's lines are printed after it, in the reference's order and formats.
Time-mean history files (QD_HISTORY=1, default 0; nothing the reference has): every QD_HISTORY_SAMPLE_EVERY-th (default 1) step of a
window of QD_HISTORY_EVERY_DAYS (default 10) planet-days -- S = max(1, int(days * day / dt + 0.5)) steps, counted on the run-local
step index from where the lane is enabled, so after a resume the windows start again at the resumed step and an open window does not
survive an autosave (QD_CHECKPOINT=1, below, carries it) -- the fields of QD_HISTORY_FIELDS (f64 planes by their Device.get names, WIND_SPEED, CURRENT_SPEED; default TS,
H, U, V, Q, CLOUD, HICE, PRECIP, ALBEDO, ISR, OLR, EFLUX, PCOND, W_LAND, S_SNOW, RUNOFF, WIND_SPEED and with the ocean SST, UO, VO, ETA,
QNET, CURRENT_SPEED; an unknown name or a field of a subsystem that is off is refused at start-up) are added into resident sums by a
fifth span lane (qingdai_amd/history.py, qd_history_*).  A chunk ends with a window's last step, behind which
<QD_OUTPUT_DIR>/history/history_day_{a}_{b}.nc (the means, n_samples, t_start_seconds, t_end_seconds, dt_seconds, sample_every,
complete) is written and one [History] line printed; a and b are the start times over `day` of the first and last sampled step,
`05.1f` like the frames (more decimals for windows shorter than 0.1 day).  The normal end of main writes the open window with
complete = 0; the signal path does not.
Per-step series (QD_SERIES=1, default 0; nothing the reference has): on every QD_SERIES_EVERY-th (default 1; the phase restarts with
each window) step of a window of QD_SERIES_EVERY_DAYS (default 10) planet-days -- history's window clock -- every field of
QD_SERIES_FIELDS (history's parser, defaults, ocean-only rule and refusals) is reduced on the device to a cos-latitude-weighted
global mean, a minimum, a maximum, a NaN count and, under QD_SERIES_ZONAL=1 (default), the zonal mean of every latitude row, in a
fixed summation order, by a sixth span lane (qingdai_amd/series.py, qd_series_*) whose records stay in a device log until the chunk
ends.  A chunk ends with a window's last step, behind which <QD_OUTPUT_DIR>/series/series_day_{a}_{b}.nc (time_seconds, step, lat,
per field {name}_mean / _min / _max / _nan [time] and {name}_zonal [time][lat], dt_seconds, sample_every, zonal, complete) is
written and one [Series] line printed, labelled like the history files.  The normal end of main writes the open window with
complete = 0; the signal path does not; under QD_CHECKPOINT=1 the checkpoint carries the open window instead.
Zonal wavenumber spectra (QD_SPECTRA=1, default 0; the reference's plan for its dissipation filters asks for them, its code has
none): on every QD_SPECTRA_EVERY-th (default 24) step of a window of QD_SPECTRA_EVERY_DAYS (default 10) planet-days -- history's
window clock -- every row of every field of QD_SPECTRA_FIELDS (default U,V,H,Q,CLOUD; history's parser, ocean-only rule and
refusals) is transformed on the device to its one-sided variance spectrum P_j(k), k = 0 .. n_lon // 2 (an f64 FFT in LDS for row
lengths 2^a 3^b 5^c, a direct DFT otherwise or under QD_SPECTRA_FORM=direct), and the rows are combined with cos-latitude weights in
a fixed order, by a seventh span lane (qingdai_amd/spectra.py, qd_spectra_*) whose records stay in a device log until the chunk ends;
under QD_SPECTRA_LAT=1 (default) the per-row powers are also summed in resident planes.  A chunk ends with a window's last step,
behind which <QD_OUTPUT_DIR>/spectra/spectra_day_{a}_{b}.nc (time_seconds, step, wavenumber, lat, per field {name}_power [time][k],
{name}_bad_rows, {name}_hi_frac [time], {name}_power_lat [lat][k], ke_power when U and V are selected, dt_seconds, sample_every,
lat_resolved, n_samples, complete) is written and one [Spectra] line printed.  The normal end of main writes the open window with
complete = 0; the signal path does not; under QD_CHECKPOINT=1 the checkpoint carries the open window and the sum planes instead.
Exact resume (QD_CHECKPOINT=1, default 0; nothing the reference has: its restart holds 14 planes as f4 and t_seconds, and the step
counters, routing buffers, tracers, carry-over planes, autotuned parameters and history window start again): every autosave --
periodic, signal, atexit, final -- also writes <QD_DATA_DIR>/checkpoint.nc (QD_CHECKPOINT_PATH names another file) behind the
reference's files, which are written exactly as before: every f64 plane as f8, the masks, the tracers, the routing buffers, the
history sums, the ecology's qd_* variables, every clock and counter, the qd_params struct and a 64-bit digest of every plane taken
on the device in one launch (qingdai_amd/checkpoint.py, qd_state_digest).  With QD_AUTOSAVE_LOAD=1 and no QD_RESTART_IN an existing
checkpoint wins over atmosphere.nc, ocean.nc, ecology.nc and plankton.nc; the file is checked on the host against its own digests,
and after the upload the device digests every plane again.  The step index continues, so the plot clock, the budget cadence, the
autotuner and the history windows fire on the steps of the uncut run, whose state the resumed run reproduces bit for bit.  A file
whose grid, ABI version, subsystem set or digests do not fit prints `[Checkpoint] refused '<path>': <reason>` and main returns 2,
unless QD_CHECKPOINT_STRICT=0 takes the load order above instead (a file refused for its subsystem set is refused behind the
routing, budget and history lanes, whose set it is checked against: those loads then run behind the lanes too, which hold nothing
the loads touch).  A checkpoint is written at span boundaries only: a SIGINT / SIGTERM that arrives inside a chunk of the device
loop is acted on behind that chunk (at most 200 steps), when the device and every host clock stand at the same step, and a save
that finds the device elsewhere than the host clocks -- atexit after an error inside a span -- prints `[Checkpoint] (reason)
skipped: ...` and leaves the last good file; the file records the step index and the device counter of the last span's end, and a
load refuses a file in which they disagree.  Refused at start-up: QD_ECO_SPECIATION=1 and a daily_hook.  With
the ecology on, ecology.nc and genes.json are written and read as under QD_ECO_PERSIST=2.  The open history window is not written
as an incomplete file at the end of main: the checkpoint carries it.
State frames (QD_STATE_PLOT=1, default 0; the same plot clock; plot_state, run_simulation.py:330-537, 2426-2428): the reference's
15-panel status figure as a mosaic of 5 x 3 tiles of n_lat x n_lon pixels -- every tile its contourf sampled at the cell centres,
with the coast, river, lake and star-position overlays, no titles, axes or colourbars -- composed on the device from the resident
state (qingdai_amd/stateframe.py, qd_stateframe_*).  A chunk ends with the firing step, which writes <QD_OUTPUT_DIR>/state_day_*.png
and a state_day_*.json with the titles, units, colormaps and levels, before the true-colour frame as in the reference.  At the end
of a chunk PRECIP, ALBEDO, EFLUX, PCOND and OLR hold the firing step's own values.  QD_PLOT_PS_MODE=abs as in
the reference.  The streamlines of the panels 7 and 8 are not drawn (their speed field is filled instead).
Ecology, plankton and ISR figures (QD_FIGURES=1, default 0; the same plot clock; plot_plankton_species, plot_isr_components and
plot_ecology, run_simulation.py:828-1060, 2430-2490): with the switch on, the reference's QD_PLOT_PHYTO (default 1, needs
plankton), QD_ECO_PLOT (default 1) and QD_PLOT_ISR (default 0) pick the figures.  Each is one row of n_lat x n_lon tiles with the
state frame's geometry and rules, composed on the device from the resident state (qingdai_amd/figures.py, qd_tiles_*): the LAI,
scalar alpha, banded alpha, canopy height and species-0 density maps (three "not available" tiles without a population); the
tracers of species 0 and 1 with the colour range of QD_PHYTO_VMAX or the 99th percentile of the ocean cells (an exact radix select
on the device); the two per-star planes with the subsolar marks and the reference's [Diagnostics] separation line.  A chunk ends
with the firing step, which writes <QD_OUTPUT_DIR>/plankton/species{0,1}_day_*.png, ecology_day_*.png and
isr_components_day_*.png, each with a .json of titles, units, colormaps, levels and marks, behind the state frame and the
true-colour frame.  A banded alpha the run has not computed yet is computed for the panel alone, as the reference does
(run_simulation.py:2458-2466); the resident map is left as it is.  A figure that fails prints one note ([PlanktonViz] / [EcologyViz]
under their diag switches) and the run goes on.
Not carried over (out of the hot path): plankton.json, plot_ocean (defined in the reference, never
called by its loop) and the diversity annotation of the ecology panel (run_simulation.py:1025-1052: it reads a name that is not
in scope there and is never drawn).

Lagrangian drifters (QD_DRIFTERS=1, default 0; nothing the reference has): QD_DRIFT_N_ATM particles on the winds and QD_DRIFT_N_OCN
on the currents (default 4096 each, Fibonacci lattice seeds, the ocean's over ocean cells; none without the ocean) are advanced on the
device on EVERY step, in index space, by an eighth span lane (qingdai_amd/drifters.py, qd_drift_*): one launch per step.  Every
QD_DRIFT_EVERY-th (default 24) step of a window of QD_DRIFT_EVERY_DAYS (default 10) planet-days -- history's window clock -- also
records positions, status, blocked counts and the values of QD_DRIFT_SAMPLE_ATM (default TS,H) / QD_DRIFT_SAMPLE_OCN (default SST) at
the particles; a chunk ends with a window's last step or where the lane's device log is full, and behind a window
<QD_OUTPUT_DIR>/drifters/drifters_day_{a}_{b}.nc is written and one [Drifters] line printed.  Under QD_CHECKPOINT=1 the particle
state and the open window travel in the checkpoint.
Flow kinematics (QD_FLOW=1, default 0; the reference defines vorticity and divergence and stops there): on every QD_FLOW_EVERY-th
(default 24) step of a window of QD_FLOW_EVERY_DAYS (default 10) planet-days -- history's window clock -- the resident (U, V) give
relative vorticity and divergence, and streamfunction and velocity potential by a Poisson solve on the device (row FFT, one
tridiagonal solve in latitude per zonal wavenumber, inverse row FFT), by a ninth span lane (qingdai_amd/flow.py, qd_flow_*): six
launches on a sampled step, one record of scalars in a device log, the four planes added into resident sum planes.  A chunk ends
with a window's last step, behind which <QD_OUTPUT_DIR>/flow/flow_day_{a}_{b}.nc (psi_mean, chi_mean, vort_mean, div_mean [lat][lon],
the scalar series [time], time_seconds, step, dt_seconds, sample_every, n_samples, complete) is written and one [Flow] line printed.
The normal end of main writes the open window with complete = 0; under QD_CHECKPOINT=1 the checkpoint carries it instead.
Spherical-harmonic power spectra (QD_SPHARM=1, default 0; nothing the reference has): on every QD_SPHARM_EVERY-th (default 24) step
of a window of QD_SPHARM_EVERY_DAYS (default 10) planet-days -- history's window clock -- every field of QD_SPHARM_FIELDS (default
VORT,DIV,H; history's parser, ocean-only rule and sampling places, and VORT, DIV: the flow lane's vorticity and divergence of the
winds) is analysed on the device into spherical-harmonic coefficients up to the triangular truncation N = min((n_lat - 1) // 2,
(n_lon - 1) // 2) (row FFT, then a Legendre recurrence fused with Clenshaw-Curtis quadrature over the latitude rows), by a tenth span
lane (qingdai_amd/spharm.py, qd_spharm_*) whose records -- power per total wavenumber, mean square, bad rows -- stay in a device log
until the chunk ends; under QD_SPHARM_2D=1 (default) the terms c_m |x_n^m|^2 are also summed in resident planes.  A chunk ends with a
window's last step, behind which <QD_OUTPUT_DIR>/spharm/spharm_day_{a}_{b}.nc is written and one [SphSpec] line printed.  The normal
end of main writes the open window with complete = 0; under QD_CHECKPOINT=1 the checkpoint carries it instead.
Eddy statistics (QD_EDDY=1, default 0; nothing the reference has): on every QD_EDDY_SAMPLE_EVERY-th (default 4) step of a window of
QD_EDDY_EVERY_DAYS (default 10) planet-days -- history's window clock -- the fields named by the pairs of QD_EDDY_PAIRS (default
U*V,V*TS,V*Q,V*H,U*U,V*V,H*H,TS*TS; names through history's field table, PRECIP and derived entries refused) give, per cell, their
deviations from an anchor and the products of the pairs, added to resident planes by a twelfth span lane (qingdai_amd/eddy.py,
qd_eddy_*; one launch per sampled step, behind the step's last).  A chunk ends with a window's last step, behind which
<QD_OUTPUT_DIR>/eddy/eddy_day_{a}_{b}.nc (per pair the zonal-mean total, mean meridional, stationary and transient parts over lat,
with QD_EDDY_MAPS=1 the transient covariance and the time means as maps) is written and one [Eddy] line printed.  The normal end of
main writes the open window with complete = 0; under QD_CHECKPOINT=1 the checkpoint carries it instead.
Extremes, spells and distributions (QD_EXTREMES=1, default 0; nothing the reference has): on every QD_EXTREMES_SAMPLE_EVERY-th
(default 4) step of a window of QD_EXTREMES_EVERY_DAYS (default 10) planet-days -- history's window clock -- the entries of
QD_EXTREMES_FIELDS (default TS,PRECIP,WIND_SPEED,H, plus SST with the ocean; history's parser) update, per cell, their maximum and
minimum with the sample they occurred in and a NaN count; the thresholds of QD_EXTREMES_THRESHOLDS (default
TS<273.15,PRECIP>1.1574e-5, i.e. freezing and 1 mm/day) their hit count, spell count and longest spell; the binned entries of
QD_EXTREMES_BINS (default PRECIP:log:1e-8:1e-2:60,TS:lin:150:350:100,WIND_SPEED:lin:0:100:100) a histogram per latitude row -- a
thirteenth span lane (qingdai_amd/extremes.py, qd_extremes_*; at most two launches per sampled step, at history's two sampling
places).  A chunk ends with a window's last step, behind which <QD_OUTPUT_DIR>/extremes/extremes_day_{a}_{b}.nc is written and one
[Extremes] line printed.  The default ranges, thresholds and cadence are guesses (the file carries the under and over shares of every
histogram).  The normal end of main writes the open window with complete = 0; under QD_CHECKPOINT=1 the checkpoint carries it.

Per iteration (run_simulation.py:1760-2340), all on the device through one qd_step_n call per chunk:
  hybrid precipitation -> clouds -> cloud tracer -> insolation -> P019 lapse/snow -> albedo -> Teq ->
  SpectralModel.time_step(Teq, dt) [no albedo argument, like the reference driver] -> ocean coupling ->
  snow commit + land bucket [-> river routing accumulation, and an event when t_accum reaches dt_hydro].
"""
from __future__ import annotations

import atexit
import importlib
import os
import signal
import sys
import time

import numpy as np

from . import SphericalGrid, SpectralModel, WindDrivenSlabOcean, OrbitalSystem, ThermalForcing, QdParams
from . import topography as topo
from .truecolor import plot_interval_steps, firing_steps      # the plot clock of the state frame, the true-colour frame and the figures

PLANET_OMEGA = 8.726646259971648e-5
# The windowed diagnostics (qingdai_amd/window_lane.py) by their NAME, which is also the Simulation attribute, the module and the
# keyword of Device.step_n.  The order of the printed lines is behaviour: WINDOW_LANES is the order in which main enables them, a
# span delivers to them and the end of a run writes their open windows; MID_RUN_FLUSH_ORDER the order in which windows that close
# on the same step are written inside a run.
WINDOW_LANES = ("history", "series", "spectra", "drifters", "flow", "spharm", "eddy", "extremes")
MID_RUN_FLUSH_ORDER = ("flow", "spharm", "eddy", "extremes", "history", "series", "spectra", "drifters")

RESTART_VARS = {  # restart name -> device field (run_simulation.py:63-124)
    "u": "U", "v": "V", "h": "H", "T_s": "TS", "cloud_cover": "CLOUD", "q": "Q", "h_ice": "HICE",
    "uo": "UO", "vo": "VO", "eta": "ETA", "Ts": "SST", "W_land": "W_LAND", "S_snow": "S_SNOW", "C_snow": "C_SNOW",
}


# ------------------------------------------------------------------------------------- NetCDF I/O
from . import ncio  # noqa: E402


def _nc_backend():
    return ncio.backend()


OCEAN_VARS = ("uo", "vo", "eta", "Ts")


def save_restart(path, grid, dev, t_seconds, land_mask, with_ocean=True):
    """run_simulation.py:63-124: dims lat/lon, every state variable AND land_mask as f4 (the reference's `wvar` writes them all
    through one f4 helper, :86-111), the ocean variables only when an ocean exists (:99-103), scalar t_seconds (f8), format=v1.
    netCDF4 when importable, else NetCDF-3 through scipy.io."""
    v = {"lat": ("f4", ("lat",), np.asarray(grid.lat, np.float32)), "lon": ("f4", ("lon",), np.asarray(grid.lon, np.float32))}
    for name, fid in RESTART_VARS.items():
        if name in OCEAN_VARS and not with_ocean:
            continue
        v[name] = ("f4", ("lat", "lon"), dev.get(fid).astype(np.float32))
    v["land_mask"] = ("f4", ("lat", "lon"), np.asarray(land_mask, np.float32))
    v["t_seconds"] = ("f8", (), float(t_seconds))
    ncio.write_nc(path, {"lat": grid.n_lat, "lon": grid.n_lon}, v,
                  {"title": "Qingdai GCM Restart", "creator": "qingdai_amd", "format": "v1"})


def load_restart(path):
    """run_simulation.py:161-183: returns {name: float32 array} + t_seconds (arrays come back f4)."""
    v, _ = ncio.read_nc(path, list(RESTART_VARS) + ["land_mask", "t_seconds"])
    out = {k: a for k, a in v.items() if k != "t_seconds"}
    out["t_seconds"] = float(v["t_seconds"]) if "t_seconds" in v else 0.0
    return out


def save_ocean(path, grid, dev, day_value=None):
    """data/ocean.nc (run_simulation.py:185-220): uo, vo, eta, Ts as f4, attribute `day`.  Never raises."""
    try:
        v = {"lat": ("f4", ("lat",), np.asarray(grid.lat, np.float32)), "lon": ("f4", ("lon",), np.asarray(grid.lon, np.float32))}
        for name, fid in (("uo", "UO"), ("vo", "VO"), ("eta", "ETA"), ("Ts", "SST")):
            v[name] = ("f4", ("lat", "lon"), dev.get(fid).astype(np.float32))
        attrs = {"title": "Qingdai Ocean State", "source": "qingdai_amd"}
        if day_value is not None:
            attrs["day"] = float(day_value)
        ncio.write_nc(path, {"lat": grid.n_lat, "lon": grid.n_lon}, v, attrs)
        return True
    except Exception as e:                                  # the reference logs and carries on
        print(f"[Ocean] Save failed: {e}")
        return False


def load_ocean(path):
    """run_simulation.py:222-246: {uo, vo, eta, Ts, day}; missing entries are None.  Never raises."""
    out = {"uo": None, "vo": None, "eta": None, "Ts": None, "day": None}
    try:
        v, attrs = ncio.read_nc(path, ["uo", "vo", "eta", "Ts"])
        out.update({k: v.get(k) for k in ("uo", "vo", "eta", "Ts")})
        out["day"] = float(attrs["day"]) if "day" in attrs else None
    except Exception as e:
        print(f"[Ocean] Load failed '{path}': {e}")
    return out


# ------------------------------------------------------------------------------------- simulation
class Simulation:
    """The reference driver's state + loop, device resident."""
    # optional members: off until __init__ or an enable_* call turns them on
    eco = indiv = daily_hook = eco_daily = indiv_daily = None
    speciation = None                      # a Speciation under QD_ECO_SPECIATION=1
    genes_export = False                   # QD_ECO_GENES_EXPORT=1 with it
    diversity_on, diversity_every, diversity_next_day = False, 10.0, 0.0
    phyto = phyto_daily = None
    routing = budget = history = None      # enable_routing, enable_budget_diag (QD_BUDGET_DIAG=1), enable_history (QD_HISTORY=1)
    series = None                          # enable_series (QD_SERIES=1)
    spectra = None                         # enable_spectra (QD_SPECTRA=1)
    drifters = None                        # enable_drifters (QD_DRIFTERS=1)
    flow = None                            # enable_flow (QD_FLOW=1)
    spharm = None                          # enable_spharm (QD_SPHARM=1)
    eddy = None                            # enable_eddy (QD_EDDY=1)
    extremes = None                        # enable_extremes (QD_EXTREMES=1)
    truecolor = stateframe = figures = None
    plot_every = None                      # the plot interval in steps, shared by the three outputs above (run_simulation.py:1649-1651)
    _failed = frozenset()                  # the non-fatal outputs whose failure has been reported
    _in_span = _in_chunk = False           # a span is in flight (_run_lanes) / a chunk of run_loop is
    _span_mark = (0, 0)                    # (step index, the device's atm counter as the host counts it) behind the bookkeeping of the
                                           # last span; a save holds the device's own counter against it (checkpoint.span_consistent)
    _stop_request = None                   # request_stop's callable
    _index_base = 0                        # the step index a resumed run started from (load_checkpoint): run_loop's clocks count on from it

    def __init__(self, n_lat=None, n_lon=None, params: QdParams | None = None, use_ocean=None, quiet=False, device=0,
                 ecology=None, individuals=None, daily_hook=None, phyto=None, speciation_rng=None):
        """ecology / individuals: None = QD_ECO_ENABLE / QD_ECO_INDIV_ENABLE (both default 1, run_simulation.py:1324,1404).
        daily_hook(sim, soil_idx, glacier_mask): the host-side daily ecology, called at planet-day boundaries.
        speciation_rng: the generator of QD_ECO_SPECIATION=1 (None = the numpy.random module, as in the reference).
        phyto: None = QD_PHYTO_ENABLE and QD_PHYTO_ADVECTION (both default 1, run_simulation.py:1347,1351)."""
        env = os.environ
        n_lat = int(n_lat if n_lat is not None else env.get("QD_N_LAT", "121"))   # run_simulation.py:1195 is 121x240
        n_lon = int(n_lon if n_lon is not None else env.get("QD_N_LON", "240"))
        self.quiet = quiet
        self.grid = SphericalGrid(n_lat, n_lon)
        # run_simulation.py:1198-1215: external topography (QD_TOPO_NC) or the procedural seed-42 planet, for
        # which the reference driver has NO elevation map (orography / lapse then see a flat bed)
        topo_nc = env.get("QD_TOPO_NC")
        self.elevation = None
        loaded = False
        if topo_nc and os.path.exists(topo_nc):
            try:
                self.elevation, self.land_mask, self.base_albedo, self.friction = topo.load_topography_from_netcdf(
                    topo_nc, self.grid, quiet=quiet)
                loaded = True
            except Exception as e:
                print(f"[Topo] Failed to load '{topo_nc}': {e}\nFalling back to procedural generation.")
        if not loaded:
            if topo_device(env):
                # QD_TOPO_DEVICE=1: the same recipe on the device (seed 42, 0.29, no overrides; no elevation map either)
                from . import topogen
                self.land_mask = topogen.generate(self.grid, seed=42, target_land_frac=0.29, device=device)["land_mask"]
            else:
                self.land_mask = topo.create_land_sea_mask(self.grid)
            self.base_albedo, self.friction = topo.generate_base_properties(self.land_mask)
            if not quiet:
                w = np.cos(np.deg2rad(self.grid.lat_mesh))
                frac = float((w * (self.land_mask == 1)).sum() / (w.sum() + 1e-15))
                print(f"[Topo] Procedural topography (seed 42). Land fraction: {frac:.3f}")
        rho_w = float(env.get("QD_RHO_W", "1000"))
        cp_w = float(env.get("QD_CP_W", "4200"))
        H_mld = float(env.get("QD_MLD_M", "50"))
        Cs_ocean = rho_w * cp_w * H_mld
        Cs_land = float(env.get("QD_CS_LAND", "3e6"))
        Cs_ice = float(env.get("QD_CS_ICE", "5e6"))
        p = params or QdParams.from_env()
        self.gcm = SpectralModel(self.grid, self.friction, H=8000, tau_rad=10 * 24 * 3600,
                                 greenhouse_factor=float(env.get("QD_GH_FACTOR", "0.40")),
                                 C_s_map=np.where(self.land_mask == 1, Cs_land, Cs_ocean).astype(float),
                                 land_mask=self.land_mask, Cs_ocean=Cs_ocean, Cs_land=Cs_land, Cs_ice=Cs_ice,
                                 params=p, device=device)
        self.dev = self.gcm._dev
        self.dev.upload_now("BASE_ALBEDO", self.base_albedo)
        if self.elevation is not None:
            self.dev.upload_now("ELEVATION", np.nan_to_num(self.elevation))
        use_ocean = (int(env.get("QD_USE_OCEAN", "1")) == 1) if use_ocean is None else bool(use_ocean)
        self.ocean = None
        if use_ocean:
            H_ocean = float(env.get("QD_OCEAN_H_M", str(H_mld)))
            self.ocean = WindDrivenSlabOcean(self.grid, self.land_mask, H_ocean,
                                             init_Ts=np.where(self.land_mask == 0, 288.0, 288.0))
        self.forcing = ThermalForcing(self.grid, OrbitalSystem())
        self.t = 0.0
        self._step_index = 0
        self._span_mark = (0, 0)                               # a fresh handle counts from zero
        self.dt = int(env.get("QD_DT_SECONDS", "300"))
        # ecology (run_simulation.py:1324-1423): adapter + canopy population + sampled individuals, state on the device
        self.daily_hook = daily_hook
        self.day_seconds = 2 * np.pi / PLANET_OMEGA
        self._accum_day = 0.0
        eco_on = (int(env.get("QD_ECO_ENABLE", "1")) == 1) if ecology is None else bool(ecology)
        if eco_on:
            from .ecology import EcologyAdapter, IndividualPool
            self.eco = EcologyAdapter(self.grid, self.land_mask, dev=self.dev)
            ind_on = (int(env.get("QD_ECO_INDIV_ENABLE", "1")) == 1) if individuals is None else bool(individuals)
            if ind_on and self.eco.pop is not None:
                self.indiv = IndividualPool(self.grid, self.land_mask, self.eco, sample_frac=0.02, per_cell=150,
                                            substeps_per_day=10, day_seconds=self.day_seconds)
            if not quiet:
                lai = f"LAI mean {self.eco.pop.summary()['LAI_mean']:.2f}" if self.eco.pop is not None else "no population (M1)"
                print(f"[Ecology] device sub-step: NB={self.eco.bands.nbands}, alpha_leaf={self.eco.alpha_leaf_scalar:.3f}, "
                      f"{lai}, individuals {self.indiv.n_indiv if self.indiv else 0}")
        # QD_ECO_DAILY=1: the daily population step as a span lane (no caller hook: a hook keeps precedence and today's behaviour)
        if eco_on and self.eco.pop is not None and daily_hook is None and eco_daily_enabled(env):
            from .ecology import PopulationDaily
            self.eco_daily = PopulationDaily(self.eco.pop, day_seconds=self.day_seconds)
            self.eco_daily.diag = int(env.get("QD_ECO_DIAG", "1")) == 1
            if not quiet:
                print(f"[Ecology] daily step on the device: K={self.eco.pop.K}, Ns={self.eco.pop.Ns}, "
                      f"spread {'on' if self.eco_daily.params.spread else 'off'}")
        # QD_ECO_SPECIATION=1: the reference's mutation draw behind every firing of that lane, the split on its resident stack
        if speciation_enabled(env, eco_daily=self.eco_daily is not None, daily_hook=daily_hook is not None):
            from .ecology import Speciation
            self.speciation = Speciation(rng=speciation_rng, env=env)
            self.genes_export = int(env.get("QD_ECO_GENES_EXPORT", "0")) == 1
            if not quiet:
                print(f"[Ecology] speciation on the device: mut_rate={self.speciation.mut_rate:g}, mut_eps={self.speciation.mut_eps:g}, "
                      f"species_max={self.speciation.species_max}, genes export {'on' if self.genes_export else 'off'}")
        # QD_ECO_INDIV_DAILY=1: IndividualPool.step_daily behind every firing of that lane
        if indiv_daily_enabled(env, eco_daily=self.eco_daily is not None, ecology=eco_on, population=eco_on and self.eco.pop is not None,
                               individuals=self.indiv is not None, daily_hook=daily_hook is not None):
            from .ecology import IndividualDaily
            self.indiv_daily = self.eco_daily.indiv_daily = IndividualDaily(self.indiv, self.eco.pop)
            if not quiet:
                print(f"[EcoIndiv] daily step on the device: {self.indiv.n_cells} cells x {self.indiv.per_cell} indiv, "
                      f"{self.indiv_daily.n_levels} levels")
        elif self.eco_daily is not None and self.indiv is not None and not quiet:
            print("[Ecology] note: IndividualPool.step_daily is not run by the device daily step.")
        # diversity diagnostics (run_simulation.py:1425-1429, 1741): the switch, the cadence, the clock's threshold in days
        if self.eco is not None and self.eco.pop is not None:
            from .ecology import diversity_env
            self.diversity_on, self.diversity_every = diversity_env(env)
        # phytoplankton tracers (run_simulation.py:1346-1364): their transport by the currents (needs the ocean), and under
        # QD_PHYTO_DAILY=1 the daily growth / optics step with its ocean-colour albedo, which the reference runs with or without the
        # ocean or the transport
        if phyto is None:
            phyto = int(env.get("QD_PHYTO_ENABLE", "1")) == 1 and int(env.get("QD_PHYTO_ADVECTION", "1")) == 1
        self.phyto_transport = bool(phyto) and self.ocean is not None
        daily_on = int(env.get("QD_PHYTO_ENABLE", "1")) == 1 and int(env.get("QD_PHYTO_DAILY", "0")) == 1
        if self.phyto_transport or daily_on:
            from .phyto import PhytoTracers
            self.phyto = PhytoTracers(self.grid, self.land_mask, dev=self.dev)
            if not quiet:
                print(f"[Phyto] resident tracers: S={self.phyto.S}, K_h={self.phyto.K_h:g} m^2/s, adv_alpha={self.phyto.adv_alpha:g}")
        if daily_on:
            from .phyto import PhytoDaily
            try:
                H_phyto = float(env.get("QD_OCEAN_H_M", env.get("QD_MLD_M", "50")))       # run_simulation.py:1354-1359
            except ValueError:
                H_phyto = 50.0
            diag = int(env.get("QD_PHYTO_DIAG", "1")) == 1
            self.phyto_daily = PhytoDaily(self.phyto, H_mld_m=H_phyto, diag=diag, dev=self.dev, day_seconds=2 * np.pi / PLANET_OMEGA)
            if diag:
                print("[Phyto] Manager initialized.")
        # banded initial surface temperature (run_simulation.py:310-328)
        if int(env.get("QD_INIT_BANDED", "0")) == 1:
            T_eq, T_pole = float(env.get("QD_INIT_T_EQ", "295.0")), float(env.get("QD_INIT_T_POLE", "265.0"))
            Ts0 = T_pole + (T_eq - T_pole) * (np.cos(np.deg2rad(self.grid.lat_mesh)) ** 2)
            self.gcm.T_s = Ts0.copy()
            if self.ocean is not None:
                self.ocean.Ts = np.where(self.land_mask == 0, Ts0, 288.0)

    # -- restart
    def load(self, path):
        rst = load_restart(path)
        for name, fid in RESTART_VARS.items():
            if name in rst and (self.ocean is not None or name not in ("uo", "vo", "eta", "Ts")):
                arr = np.asarray(rst[name], dtype=np.float64)        # arrives as f4, like the reference
                if name == "cloud_cover":
                    arr = np.clip(arr, 0.0, 1.0)
                if name == "h_ice":
                    arr = np.maximum(arr, 0.0)
                self.dev.set(fid, arr)
        self.t = float(rst.get("t_seconds", 0.0))

    def save(self, path):
        save_restart(path, self.grid, self.dev, self.t, self.land_mask, with_ocean=self.ocean is not None)

    # -- exact resume (qingdai_amd/checkpoint.py)
    def save_checkpoint(self, path, reason=None):
        """Write the whole resident state, every clock and the device digests to `path` (temporary name, then os.replace) -> the run
        digest.  Unlike `save`, a fresh Simulation that loads the file continues this run bit for bit."""
        from . import checkpoint
        return checkpoint.save(self, path, reason=reason)

    def load_checkpoint(self, path, env=None):
        """Put `path` back into this freshly built Simulation (its routing, budget and history lanes enabled as in the saved run) ->
        the run digest.  Raises checkpoint.CheckpointRefused, with nothing touched, when the file does not fit the run."""
        from . import checkpoint
        return checkpoint.load(self, path, env=env)

    def digest(self):
        """{plane name: 64-bit digest} of every resident plane of the checkpoint set, taken on the device in one call, plus "run",
        the digest of the digests: two runs are in the same state exactly when these agree."""
        from . import checkpoint
        return checkpoint.simulation_digest(self)

    def load_ocean_override(self, path):
        """run_simulation.py:1497-1509 / 1542-1553: QD_LOAD_OCEAN=1 (default) lets a standardized data/ocean.nc override the ocean
        fields after the atmosphere checkpoint was read.  Returns True when something was loaded."""
        if self.ocean is None or not os.path.exists(path):
            return False
        v, _ = ncio.read_nc(path, list(OCEAN_VARS))
        for name in OCEAN_VARS:
            if name in v:
                self.dev.set(RESTART_VARS[name], np.asarray(v[name], dtype=np.float64))
        return bool(v)

    def save_autosave(self, data_dir="data"):
        """run_simulation.py:248-304 + 126-159 + 185-220: data/atmosphere.nc (the restart layout with the epoch
        in t_seconds), under QD_ECO_PERSIST >= 1 data/ecology.nc and data/genes.json, then data/ocean.nc, data/topography.nc."""
        day = self.t / (2 * np.pi / PLANET_OMEGA)
        save_restart(os.path.join(data_dir, "atmosphere.nc"), self.grid, self.dev, self.t, self.land_mask, with_ocean=self.ocean is not None)
        self.save_ecology(data_dir, day)
        if self.ocean is not None:
            save_ocean(os.path.join(data_dir, "ocean.nc"), self.grid, self.dev, day_value=day)
        topo.export_topography_to_netcdf(os.path.join(data_dir, "topography.nc"), self.grid, self.land_mask, self.base_albedo,
                                         self.friction, elevation=self.elevation)
        if self.phyto_daily is not None:                        # run_simulation.py:1677-1685, the reference's variable set
            self.phyto_daily.save_distribution_nc(os.path.join(data_dir, "plankton.nc"), day_value=day)
        elif self.phyto is not None:                            # (the tracer part of plankton.nc)
            self.phyto.save_distribution_nc(os.path.join(data_dir, "plankton.nc"), day_value=day)

    def save_ecology(self, data_dir="data", day_value=None, env=None):
        """run_simulation.py:274-304 under QD_ECO_PERSIST >= 1: ecology.nc -- at QD_ECO_AUTOSAVE_PATH when that ends in `.nc`, else
        <data>/ecology.nc -- through EcologyAdapter.save_autosave, then <data>/genes.json.  A failure prints the reference's line and
        never stops the run -> the path written, or None."""
        env = os.environ if env is None else env
        if eco_persist_level(env) < 1 or self.eco is None or self.eco.pop is None:
            return None
        try:
            path_env = env.get("QD_ECO_AUTOSAVE_PATH")
            path = path_env if (path_env and path_env.lower().endswith(".nc")) else os.path.join(data_dir, "ecology.nc")
            try:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            except Exception:      # noqa: BLE001
                pass
            ok = False
            try:
                ok = bool(self.eco.save_autosave(path, day_value=float(day_value), extended=eco_persist_level(env) == 2, indiv=self.indiv))
                if not ok:
                    print(f"[Autosave] Ecology extended save returned False for '{path}'")
            except Exception as e:      # noqa: BLE001
                print(f"[Autosave] Ecology extended save failed: {e}")
            try:
                self.eco.save_genes_json(os.path.join(data_dir, "genes.json"), day_value=float(day_value))
            except Exception:      # noqa: BLE001
                pass
            return path if ok else None
        except Exception as e:      # noqa: BLE001
            print(f"[Autosave] Ecology save failed: {e}")
            return None

    def load_ecology(self, data_dir="data", env=None):
        """run_simulation.py:1464-1488 / 1566-1590 under QD_ECO_PERSIST >= 1 and QD_AUTOSAVE_LOAD=1 (default): genes.json first (from
        QD_ECO_GENES_JSON_PATH or <data>/genes.json), then the ecology file (QD_ECO_AUTOSAVE_PATH -- any extension -- or
        <data>/ecology.nc) with QD_ECO_ON_MISMATCH, and the reference's lines under QD_ECO_DIAG -> True when the state was loaded."""
        env = os.environ if env is None else env
        if eco_persist_level(env) < 1 or self.eco is None or int(env.get("QD_AUTOSAVE_LOAD", "1")) != 1:
            return False
        diag = int(env.get("QD_ECO_DIAG", "1")) == 1
        try:
            genes_path = env.get("QD_ECO_GENES_JSON_PATH") or os.path.join(data_dir, "genes.json")
            if os.path.exists(genes_path):
                self.eco.load_genes_json(genes_path)
        except Exception as e:      # noqa: BLE001
            if diag:
                print(f"[Ecology] genes autosave load skipped: {e}")
        ok = False
        try:
            eco_path = env.get("QD_ECO_AUTOSAVE_PATH") or os.path.join(data_dir, "ecology.nc")
            if os.path.exists(eco_path):
                ok = bool(self.eco.load_autosave(eco_path, on_mismatch=env.get("QD_ECO_ON_MISMATCH", "fallback"), indiv=self.indiv,
                                                        extended=eco_persist_level(env) == 2))
                if diag:
                    print(f"[Ecology] autosave load {'OK' if ok else 'failed'} from '{eco_path}'")
        except Exception as e:      # noqa: BLE001
            if diag:
                print(f"[Ecology] autosave load skipped: {e}")
        return ok

    # -- the loop
    def bootstrap_ecology(self):
        """run_simulation.py:1716-1726: one step_subdaily on the t = 0 insolation before the loop starts."""
        if self.eco is None or not self.eco.params.albedo_couple:
            return
        self.forcing.update_device(0.0, with_teq=False)
        self.eco.step_subdaily(None, None, float(self.dt))

    def _daily(self):
        """The day-boundary block of run_simulation.py:1786-1864 for the ecology: soil index from W_land, zero on ice sheets."""
        if self.daily_hook is None:
            return
        cap = float(os.environ.get("QD_ECO_SOIL_WATER_CAP", "50.0"))
        for k in ("W_LAND", "GLACIER"):
            self.dev._host.pop(k, None)
        glacier = self.dev.get("GLACIER") != 0.0
        soil_idx = np.clip(self.dev.get("W_LAND") / max(1e-6, cap), 0.0, 1.0) * (~glacier)
        self.daily_hook(self, soil_idx, glacier)

    def run_steps(self, n):
        """n iterations of run_simulation.py:1760-2340 as resident qd_step_n calls: one per stretch between planet-day
        boundaries when a daily ecology hook is installed (the hook runs where the reference runs eco.step_daily, i.e. before
        the rest of the step that completes the day), one per QD_ENERGY_TUNE_EVERY steps when the autotuner is on."""
        if n <= 0:
            return
        if self.eco is not None and self.daily_hook is not None:
            left = n
            while left > 0:
                a, k = self._accum_day, 0                      # run_simulation.py:1784-1786: accum += dt; while accum >= day
                while k < left and a + self.dt < self.day_seconds:
                    a += self.dt
                    k += 1
                if k > 0:
                    self._run_span(k)
                    self._accum_day = a
                    left -= k
                    continue
                self._accum_day += self.dt
                while self._accum_day >= self.day_seconds:
                    self._accum_day -= self.day_seconds
                    self._daily()
                self._run_span(1)
                left -= 1
            return
        self._run_span(n)

    def _run_span(self, n):
        p = self.dev.params
        autotune = (int(p.gh_lock) == 0) and int(os.environ.get("QD_ENERGY_AUTOTUNE", "0")) == 1 and self.ocean is not None
        if autotune:                                           # run_simulation.py:1256-1257, 2242-2246
            # the reference evaluates the budget inside step i (i % every == 0), after time_step, and the nudged
            # parameters first act on step i+1: run that step on its own with the in-step diagnostics, then the rest
            from . import energy as _energy
            every = max(1, int(os.environ.get("QD_ENERGY_TUNE_EVERY", "50")))
            left = n
            while left > 0:
                if self._step_index % every == 0:
                    self._run_chunk(1, energy_diag=True)
                    _energy.autotune_greenhouse_params(p, self.dev.energy_diagnostics_last())
                    self.dev.push_params()
                    left -= 1
                    continue
                k = min(left, every - (self._step_index % every))
                self._run_chunk(k)
                left -= k
            return
        self._run_chunk(n)

    @property
    def t(self):
        """Model time in seconds.  Assigning it (a restart, an epoch) makes the value the origin the following steps count from."""
        return self._t

    @t.setter
    def t(self, value):
        self._t = float(value)
        self._t_origin = (self._t, 0, None)                    # (t0, steps since, their dt)

    def _span_times(self, n, advance=True):
        """The times of the next n steps as the reference's `np.arange(t0, t0 + duration, dt)` holds them (run_simulation.py:1639):
        t0 + i * ((t0 + dt) - t0) with i counted from the origin, not from the span -- so that the insolation and the phytoplankton
        firing test see the same float64 times however the run is cut into spans -> (times [n], the time after them).
        advance=False only looks ahead: the origin stays where it is."""
        t0, k, dt = self._t_origin
        if dt is not None and dt != float(self.dt):            # the step changed: count afresh from where the clock stands
            t0, k = self._t, 0
        delta = (t0 + float(self.dt)) - t0
        if advance:
            self._t_origin = (t0, k + n, float(self.dt))
        return t0 + (k + np.arange(n)) * delta, float(t0 + (k + n) * delta)

    # -- outputs that fire behind a chunk's last step (run_simulation.py:2404-2490)
    def _nonfatal(self, fn, note, key=None, cleanup=None):
        """An output never stops the run, like the reference's plotting: fn() -> its result, or None after a failure.  `note`
        (a format of the exception; None = silent) is printed once per `key`, every time without one; `cleanup` runs behind it."""
        try:
            return fn()
        except Exception as e:      # noqa: BLE001
            if note is not None and key not in self._failed:
                print(note.format(e))
            if key is not None:
                self._failed |= {key}
            if cleanup is not None:
                cleanup()
            return None

    def diversity_due(self, n_max):
        """Looks at the next n_max steps with the reference's clock -> (steps up to and including the first firing step, that
        step's start time in days), or (None, None) when none of them fires or the diagnostics are off."""
        if not self.diversity_on or n_max <= 0:
            return None, None
        from .ecology import diversity_firings
        times, _ = self._span_times(int(n_max), advance=False)
        fired, _ = diversity_firings(times, self.day_seconds, self.diversity_next_day, self.diversity_every)
        if not fired:
            return None, None
        return fired[0] + 1, float(times[fired[0]]) / self.day_seconds

    def run_diversity(self, t_days, output_dir=None):
        """One firing on the state as it stands (the end of the firing step): the device diagnostics, the reference's files under
        <output_dir>/ecology/ named by t_days, the clock's next threshold.  A failure is reported once and never stops the run."""
        from .ecology import write_diversity_files, diversity_line
        self.diversity_next_day = t_days + self.diversity_every
        diag = int(os.environ.get("QD_ECO_DIAG", "1")) == 1

        def fire():
            alpha_map, bc_local, L_s, summary = self.eco.pop.diversity()
            out = output_dir if output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")
            write_diversity_files(out, t_days, alpha_map, bc_local, L_s, summary, self.land_mask)
            if diag:
                print(diversity_line(t_days, summary))
            return summary
        return self._nonfatal(fire, "[Diversity] diagnostics skipped: {}" if diag else None, "diversity")

    def enable_truecolor(self, env=None):
        """QD_TRUECOLOR=1: the renderer on this run's device and the reference's plot interval -> the TrueColor or None."""
        env = os.environ if env is None else env
        self.truecolor = None
        if int(env.get("QD_TRUECOLOR", "0")) == 1:
            from .truecolor import TrueColor
            self.truecolor = TrueColor(self)
            self.plot_every = plot_interval_steps(env, self.dt)
        return self.truecolor

    def enable_stateframe(self, env=None):
        """QD_STATE_PLOT=1: the state-frame renderer on this run's device, configured at once (a latitude-band handle is refused
        here), and the reference's plot interval -> the StateFrame or None."""
        env = os.environ if env is None else env
        self.stateframe = None
        if int(env.get("QD_STATE_PLOT", "0")) == 1:
            from .stateframe import StateFrame
            sf = StateFrame(self, env=env)                     # QD_PLOT_PS_MODE and the river variables from the same mapping
            sf.configure()
            self.stateframe = sf
            self.plot_every = plot_interval_steps(env, self.dt)
        return self.stateframe

    def enable_figures(self, env=None):
        """QD_FIGURES=1: the tile renderer on this run's device, configured at once (a latitude-band handle is refused here), and
        the reference's plot interval -> the Figures or None.  QD_PLOT_PHYTO, QD_ECO_PLOT and QD_PLOT_ISR then pick the figures."""
        env = os.environ if env is None else env
        self.figures = None
        from .figures import Figures, figures_enabled
        if figures_enabled(env):
            fg = Figures(self, env=env)
            fg.configure()
            self.figures = fg
            self.plot_every = plot_interval_steps(env, self.dt)
        return self.figures

    def plot_due(self, i0, n_max):
        """Looks at the next n_max steps, the first of which has the run-local index i0, with the plot clock the state frame, the
        true-colour frame and the figures share -> (steps up to and including the first firing step, that step's start time in
        days), or (None, None) when none of them fires or none of the three is on."""
        if self.plot_every is None or n_max <= 0:
            return None, None
        fired = firing_steps(i0, n_max, self.plot_every)
        if not fired:
            return None, None
        times, _ = self._span_times(fired[0] + 1, advance=False)
        return fired[0] + 1, float(times[fired[0]]) / self.day_seconds

    def run_truecolor(self, t_days, output_dir=None):
        """One firing on the state as it stands (the end of the firing step): the frame file and the [TrueColor] line."""
        def fire():
            path, line = self.truecolor.write_frame(t_days, output_dir)
            print(line)
            return path
        return self._nonfatal(fire, "[TrueColor] frame skipped: {}", "truecolor")

    def run_stateframe(self, t_days, output_dir=None):
        """One firing on the state as it stands (the end of the firing step): state_day_*.png and its .json."""
        return self._nonfatal(lambda: self.stateframe.write_frame(t_days, output_dir), "[StatePlot] frame skipped: {}", "stateframe")

    def figure_names(self, env=None):
        """The figures this run writes, in their order (run_simulation.py:2431, 2469, 2489)."""
        from .figures import read_env
        e = read_env(self.figures.env if env is None else env)
        return ([n for n, on in (("plankton", e["plot_phyto"] and self.phyto is not None), ("ecology", e["plot_eco"]), ("ISR", e["plot_isr"])) if on],
                e)

    def run_figures(self, t_days, output_dir=None):
        """One firing on the state as it stands (the end of the firing step): the plankton maps, the ecology panel, the ISR figure,
        each with its .json.  A failure prints one note per figure -- the reference's [PlanktonViz] / [EcologyViz] lines under their
        diag switches -- and never stops the run."""
        fg = self.figures
        names, e = self.figure_names()
        done = []
        for name, fn, note in (("plankton", lambda: fg.write_plankton(t_days, output_dir), "[PlanktonViz] skipped: {}" if e["phyto_diag"] else None),
                               ("ecology", lambda: fg.write_ecology(t_days, output_dir), "[EcologyViz] skipped: {}" if e["eco_diag"] else None),
                               ("ISR", lambda: fg.write_isr(t_days, output_dir, echo=print)[0], "[ISRViz] figure skipped: {}")):
            if name in names:
                self._nonfatal(lambda: done.append(fn()), note, name)
        return done

    def outputs_due(self, i0, n_max):
        """The outputs that fire within the next n_max steps, the first of which has the run-local index i0, in the order the
        reference writes them (run_simulation.py:2404-2490: diversity, plot_state, plot_true_color, then the plankton, ecology
        and ISR figures) -> [(steps up to and including the firing step, that step's start time in days, the run_* to call)]."""
        plot = self.plot_due(i0, n_max)
        due = [(self.diversity_due(n_max), self.run_diversity)]
        due += [(plot, run) for on, run in ((self.stateframe, self.run_stateframe), (self.truecolor, self.run_truecolor),
                                            (self.figures, self.run_figures)) if on is not None]
        return [(k, day, run) for (k, day), run in due if k is not None]

    def run_loop(self, n_total, next_autosave_t=None, after_chunk=None):
        """n_total steps in chunks of at most 200 (chunk_until), each ending no later than the next autosave threshold's step and
        the first step that fires an output; the outputs due on a chunk's last step run behind it, in outputs_due's order (two
        cadences may fall on one step).  after_chunk(done, next_autosave_t) -> the threshold for the chunks that follow."""
        done = 0
        while done < n_total:
            self._in_chunk = True                              # a stop asked for in here (request_stop) waits for the chunk's end
            try:
                due = self.outputs_due(self._index_base + done, min(200, n_total - done))
                n = chunk_until(self.t, self.dt, next_autosave_t, n_total - done, fire_in=min((k for k, _, _ in due), default=None))
                self.run_steps(n)
                done += n
                for k, t_days, run in due:
                    if n == k:                                 # the chunk ended with the firing step
                        run(t_days)
                if after_chunk is not None:
                    next_autosave_t = after_chunk(done, next_autosave_t)
            finally:
                self._in_chunk = False
            if self._stop_request is not None:                 # every clock, delivery, window file and output of the chunk is done
                stop, self._stop_request = self._stop_request, None
                stop()

    def request_stop(self, stop):
        """Called from a signal handler that wants a consistent state: inside a chunk of run_loop -> True, and stop() is called
        behind that chunk (at most 200 steps), when the device and every host clock stand at the same step; else -> False and
        the caller acts at once."""
        if not self._in_chunk:
            return False
        self._stop_request = stop
        return True

    # -- speciation (adapter.py:437-466 inside run_simulation.py:1786-1864)
    def speciation_due(self, n_max):
        """Walks the daily firings of the next n_max steps in firing order, one rand() per firing (kept by firing number, so a
        second look never draws again), and stops drawing at the first hit -> the steps BEFORE the hit's step (the chunk that may
        run with the lane; 0 when the very next step holds the hit), or None when none of them holds one or the switch is off."""
        spec = self.speciation
        if spec is None or n_max <= 0 or not spec.mut_rate > 0.0:
            return None
        from .ecology import daily_counts
        fire, _ = daily_counts(self.eco_daily.accum_day, float(self.dt), int(n_max), self.eco_daily.day_seconds)
        k = 0
        for i, c in enumerate(fire.tolist()):
            for _ in range(c):
                k += 1
                if spec.hit_ahead(k):
                    return i
        return None

    def _speciation_step(self, energy_diag=False):
        """The step that holds a hit: its firings are taken one by one through the lane's class seam (qd_eco_daily_step on the
        resident soil water, what an in-span firing runs), each followed by the reference's draw and, on a hit, the event -- all
        BEFORE the rest of the step, as in the reference, whose day-boundary block then refreshes the banded alpha
        (run_simulation.py:1837-1846; here under QD_ECO_BANDS_COUPLE=1, on a hit).  The step then runs with these firings struck
        out of the lane's schedule; the day accumulator advances as always."""
        from .ecology import daily_counts
        lane, spec = self.eco_daily, self.speciation
        fire, _ = daily_counts(lane.accum_day, float(self.dt), 1, lane.day_seconds)
        a = np.float64(lane.accum_day) + np.float64(self.dt)
        t_i = float(self._span_times(1, advance=False)[0][0])
        for _ in range(int(fire[0])):
            a = a - np.float64(lane.day_seconds)
            self.dev.eco_daily_step(None)
            lane._fired(1)
            lane.span_deliver(float(self.dt))
            if spec.event(self.eco) is not None and self.eco.params.bands_couple:
                self.eco.banded_alpha()
            self._export_genes(t_i, float(a))
        lane.struck = int(fire[0])
        self._run_cut(1, energy_diag)

    def _export_genes(self, t_i, accum_after):
        """QD_ECO_GENES_EXPORT=1: genes_day_*.json of one firing, named by (t_i - accum_after) / day (run_simulation.py:1847-1861:
        twice under QD_ECO_BANDS_COUPLE=1, behind the banded update and again behind it, like the reference)."""
        if not self.genes_export:
            return
        out = os.environ.get("QD_OUTPUT_DIR", "output")
        day_value = float((t_i - accum_after) / self.day_seconds)
        for _ in range(2 if self.eco.params.bands_couple else 1):
            self.eco.export_genes(out, day_value)

    def _run_chunk(self, n, energy_diag=False):
        """n steps; under QD_ECO_SPECIATION=1 cut so that a chunk ends with the step BEFORE one that holds a hit."""
        while self.speciation is not None and n > 0:
            k = self.speciation_due(n)
            if k is None:
                break
            if k > 0:
                self._run_cut(k, energy_diag)
            self._speciation_step(energy_diag)
            n -= k + 1
        if n > 0:
            self._run_cut(n, energy_diag)

    def _run_cut(self, n, energy_diag=False):
        """n steps through _run_lanes, cut so that a chunk ends with the last step of a window of every windowed lane that is on,
        behind which the window's file is written (and the next window starts from zero)."""
        on = self._window_lanes()
        while n > 0:
            k = min([n] + [lane.steps_to_window_end() for lane in on.values()])      # (the drifters': or the step that fills their log)
            self._run_lanes(k, energy_diag)
            n -= k
            for name in MID_RUN_FLUSH_ORDER:
                if name in on and on[name].window_closed():
                    getattr(self, "flush_" + name)()

    def _window_lanes(self):
        """{name: lane} of the windowed lanes that are on, in WINDOW_LANES' order."""
        lanes = {name: getattr(self, name, None) for name in WINDOW_LANES}
        return {name: lane for name, lane in lanes.items() if lane is not None}

    def flush_window(self, name, complete=1):
        """Write the open window of the lane `name` -> the path or None.  A failure is reported and the window is dropped (the next
        one starts from zero): output never stops the run."""
        lane = getattr(self, name)
        return self._nonfatal(lambda: lane.flush(complete=complete), f"[{lane.TAG}] window skipped: {{}}", cleanup=lane.drop)

    def flush_history(self, complete=1):
        return self.flush_window("history", complete)

    def flush_series(self, complete=1):
        return self.flush_window("series", complete)

    def flush_spectra(self, complete=1):
        return self.flush_window("spectra", complete)

    def flush_drifters(self, complete=1):
        return self.flush_window("drifters", complete)

    def flush_flow(self, complete=1):
        return self.flush_window("flow", complete)

    def flush_spharm(self, complete=1):
        return self.flush_window("spharm", complete)

    def flush_eddy(self, complete=1):
        return self.flush_window("eddy", complete)

    def flush_extremes(self, complete=1):
        return self.flush_window("extremes", complete)

    def _run_lanes(self, n, energy_diag=False):
        """One span: the lanes that are on, qd_step_n, the clock, each lane's lines (phyto, routing, budget, eco daily with the
        individuals')."""
        origin = self._t_origin
        times, t_next = self._span_times(n)
        stars = self.forcing.star_table(times)
        eco_daily = self.eco_daily if self.daily_hook is None else None
        if self.budget is not None:
            self.budget.routed = self.routing is not None
        lanes = {k: p for k, p in (("phyto_daily", self.phyto_daily), ("routing", self.routing), ("budget", self.budget),
                                   ("eco_daily", eco_daily)) if p is not None}
        lanes.update(self._window_lanes())
        eco_clock = eco_daily.span_clock() if eco_daily is not None else None
        # from here to the end of the bookkeeping the device and the host clocks disagree: what interrupts in between (a signal
        # handler runs right behind the device call) must not take the state for a span boundary (checkpoint.span_consistent)
        self._in_span = True
        try:
            self.dev.step_n(stars, float(self.dt), with_ocean=self.ocean is not None, with_physics=True, pass_albedo=False,
                            with_hydrology=True, energy_diag=energy_diag, ecology=self.eco is not None, phyto=self.phyto_transport,
                            t0=times, **lanes)
        except Exception:
            self._t_origin = origin                            # nothing ran: the clock stays where it was, like the lanes' clocks
            self._in_span = False                              # (where the device did run a part of it, the span mark no longer fits)
            raise
        self._t = t_next
        self._step_index += n
        for p in lanes.values():
            recs = p.span_deliver(float(self.dt))              # the span's lines, oldest first
            if p is eco_daily and self.speciation is not None and len(recs):
                self._firings_passed(len(recs), times, *eco_clock)
        self._span_mark = (self._step_index, self._span_mark[1] + n)      # qd_step_n moves the device's atm counter by one per step
        self._in_span = False

    def _firings_passed(self, n_fired, times, accum0, struck0):
        """Behind a span's eco-daily firings under QD_ECO_SPECIATION=1: none of them was a hit, and the weights and genes are the
        chunk's -- so QD_ECO_GENES_EXPORT=1 writes every firing's file now, but for those the host ran before the span."""
        self.speciation.passed(n_fired)
        if not self.genes_export:
            return
        from .ecology import daily_counts
        day = self.eco_daily.day_seconds
        fire, _ = daily_counts(accum0, float(self.dt), len(times), day)
        a = np.float64(accum0)
        for i in range(len(times)):
            a = a + np.float64(self.dt)
            for q in range(int(fire[i])):
                a = a - np.float64(day)
                if not (i == 0 and q < struck0):
                    self._export_genes(float(times[i]), float(a))

    def enable_budget_diag(self, env=None):
        """QD_BUDGET_DIAG=1: the reference's periodic budget lines ([EnergyDiag], [OceanE], [OceanDiag], [HumidityDiag],
        [WaterDiag], [HydroRoutingDiag]) from a device lane (qingdai_amd/budget_diag.py) -> the BudgetDiag or None.  The run-local
        step index the reference's `i % 200` counts starts where this is called."""
        from .budget_diag import from_env
        self.budget = from_env(self.dev, self.grid, os.environ if env is None else env, with_ocean=self.ocean is not None,
                               routed=self.routing is not None)
        return self.budget

    def _enable_window(self, name, env=None):
        """QD_<NAME>=1: the windowed lane `name` (qingdai_amd/<name>.py), kept by a device lane and written per window to
        <QD_OUTPUT_DIR>/<name>/ -> the lane or None.  The run-local step index the windows count on starts where this is called.
        An unknown field name raises here, before the loop."""
        env = os.environ if env is None else env
        from_env = importlib.import_module("." + name, __package__).from_env
        if name == "drifters":
            lane = from_env(self, env)
        else:
            kw = {} if name == "flow" else {"with_ocean": self.ocean is not None}
            lane = from_env(self.dev, self.grid, env, dt=float(self.dt), day=self.day_seconds, **kw)
        setattr(self, name, lane)
        return lane

    def enable_history(self, env=None):
        """QD_HISTORY=1: time means of the selected fields."""
        return self._enable_window("history", env)

    def enable_series(self, env=None):
        """QD_SERIES=1: per-step global means, extrema, NaN counts and zonal means."""
        return self._enable_window("series", env)

    def enable_spectra(self, env=None):
        """QD_SPECTRA=1: zonal wavenumber spectra."""
        return self._enable_window("spectra", env)

    def enable_flow(self, env=None):
        """QD_FLOW=1: vorticity, divergence, streamfunction and velocity potential of the winds."""
        return self._enable_window("flow", env)

    def enable_spharm(self, env=None):
        """QD_SPHARM=1: spherical-harmonic power spectra."""
        return self._enable_window("spharm", env)

    def enable_extremes(self, env=None):
        """QD_EXTREMES=1: per-cell extremes, threshold frequencies and spells, per-row histograms."""
        return self._enable_window("extremes", env)

    def enable_eddy(self, env=None):
        """QD_EDDY=1: covariances and transports of the selected pairs of fields."""
        return self._enable_window("eddy", env)

    def enable_drifters(self, env=None):
        """QD_DRIFTERS=1: Lagrangian drifters on the winds and the currents."""
        return self._enable_window("drifters", env)

    def enable_routing(self, env=None):
        """run_simulation.py:1294-1321 with the reference's QD_HYDRO_* defaults and messages -> the RiverRouting or None."""
        env = os.environ if env is None else env
        self.routing = None
        try:
            enabled, net, dt_h, diag = hydro_env(env)
            if not enabled:
                print("[HydroRouting] Disabled by QD_HYDRO_ENABLE=0.")
                return None
            if not (net and os.path.exists(net)):
                # QD_HYDRO_AUTOGEN=1: the reference's _try_autogen_hydro_network (run_simulation.py:1063-1127), on the device
                if hydro_autogen(env):
                    self.autogen_network(net, env)
                if not (net and os.path.exists(net)):
                    print(f"[HydroRouting] Enabled but network not available; running WITHOUT routing "
                          f"(QD_HYDRO_NETCDF='{net}').")
                    return None
            from .routing import RiverRouting
            self.routing = RiverRouting(self.grid, net, dt_hydro_hours=dt_h,
                                        treat_lake_as_water=(int(env.get("QD_TREAT_LAKE_AS_WATER", "1")) == 1),
                                        alpha_lake=(float(env["QD_ALPHA_LAKE"]) if env.get("QD_ALPHA_LAKE") else None),
                                        diag=diag, dev=self.dev)
            print(f"[HydroRouting] Enabled with network '{net}'.")
        except Exception as e:      # noqa: BLE001  (the reference never lets routing stop the run)
            print(f"[HydroRouting] Initialization skipped due to error: {e}")
            self.routing = None
        return self.routing

    def autogen_network(self, path, env=None):
        """run_simulation.py:1063-1127: build the network from the run's own land mask and elevation (zeros for the procedural
        planet) with eps 1e-3 and 200 sweeps (qingdai_amd/hydronet.py, on this handle) and write it to `path` -> True on
        success.  Failures print the reference's message and return False."""
        env = os.environ if env is None else env
        try:
            from .hydronet import generate_network, write_network
            topo_nc = env.get("QD_TOPO_NC")
            src = "procedural" if (not topo_nc or not os.path.exists(str(topo_nc))) else os.path.basename(str(topo_nc))
            print(f"[HydroRouting] Auto-generating network to '{path}' (source={src})...")
            t0 = time.perf_counter()
            net = generate_network(self.grid, self.land_mask, self.elevation, eps=1e-3, max_iters=200, dev=self.dev)
            write_network(path, self.grid, net, auto=True)
            print("[HydroRouting] Network auto-generation complete.")
            print(f"[HydroNet] built on the device in {time.perf_counter() - t0:.2f} s: {net['sweeps']} pit-fill sweeps, "
                  f"{net['n_lakes']} lakes.")
            return True
        except Exception as e:      # noqa: BLE001  (the reference goes on without routing)
            print(f"[HydroRouting] Auto-generation failed: {e}")
            return False

    def diagnostics(self):
        d = self.dev
        from ._lib import R_MAXABS, R_COSMEAN
        return {"max|u|": d.reduce("U", R_MAXABS), "max|v|": d.reduce("V", R_MAXABS), "max|h|": d.reduce("H", R_MAXABS),
                "<T_s>": d.reduce("TS", R_COSMEAN), "<cloud>": d.reduce("CLOUD", R_COSMEAN),
                "<E>": d.reduce("EFLUX", R_COSMEAN), "<P>": d.reduce("PRECIP", R_COSMEAN)}


def hydro_env(env):
    """-> (enabled, network path, dt_hydro hours, diag) from QD_HYDRO_ENABLE / QD_HYDRO_NETCDF / QD_HYDRO_DT_HOURS / QD_HYDRO_DIAG
    with the reference's defaults (run_simulation.py:1297-1314)."""
    return (int(env.get("QD_HYDRO_ENABLE", "1")) == 1, env.get("QD_HYDRO_NETCDF", "data/hydrology.nc"),
            float(env.get("QD_HYDRO_DT_HOURS", "6")), int(env.get("QD_HYDRO_DIAG", "1")) == 1)


def eco_daily_enabled(env):
    """QD_ECO_DAILY (default 0): 1 runs the daily population step on the device.  Refuses QD_ECO_MUT_RATE > 0 without
    QD_ECO_SPECIATION=1: the reference's speciation draws from the global NumPy generator after every daily step, which the device
    step alone does not restate."""
    if int(env.get("QD_ECO_DAILY", "0")) != 1:
        return False
    try:
        mut = float(env.get("QD_ECO_MUT_RATE", "0.0"))
    except ValueError:
        mut = 0.0
    if mut > 0.0 and not _speciation_switch(env):
        raise ValueError(f"QD_ECO_DAILY=1 does not support QD_ECO_MUT_RATE > 0 (got {mut:g}): stochastic speciation is host code "
                         "outside the device daily step; unset one of the two")
    return True


def _speciation_switch(env):
    try:
        return int(env.get("QD_ECO_SPECIATION", "0")) == 1
    except ValueError:
        return False


def speciation_enabled(env, *, eco_daily, daily_hook):
    """QD_ECO_SPECIATION (default 0): 1 runs the reference's speciation (adapter.py:437-515) behind the device daily vegetation
    step: QD_ECO_MUT_RATE, QD_ECO_MUT_EPS, QD_ECO_SPECIES_MAX, QD_ECO_MUT_LAMBDA_DRIFT and QD_ECO_GENES_EXPORT as the reference
    reads them.  Refused at start-up without what it stands on, and where the reference's behaviour is not restated."""
    if not _speciation_switch(env):
        return False
    missing = [what for ok, what in ((eco_daily, "QD_ECO_DAILY=1 with QD_ECO_ENABLE=1 and a population"), (not daily_hook, "no daily_hook")) if not ok]
    if missing:
        raise ValueError("QD_ECO_SPECIATION=1 needs " + ", ".join(missing) + ": the event runs on the resident stack of the device "
                         "daily vegetation step; set what is missing or unset QD_ECO_SPECIATION")
    if int(env.get("QD_ECO_INDIV_DAILY", "0")) == 1:
        raise ValueError("QD_ECO_SPECIATION=1 does not run with QD_ECO_INDIV_DAILY=1: the individuals were sampled for the run's "
                         "species; unset one of the two")
    from .ecology import Speciation
    probe = Speciation(env=env)
    if not probe.mut_eps > 0.0:
        raise ValueError(f"QD_ECO_SPECIATION=1 needs QD_ECO_MUT_EPS > 0 (got {probe.mut_eps:g}): with nothing to split the reference "
                         "adds no species and truncates its gene table (adapter.py:456-460), which is not restated")
    if probe.species_max > 64:
        raise ValueError(f"QD_ECO_SPECIATION=1 needs QD_ECO_SPECIES_MAX <= 64 (got {probe.species_max}): the resident stack holds at "
                         "most 64 species")
    return True


def eco_persist_level(env):
    """QD_ECO_PERSIST (default 0): 1 writes and reads data/ecology.nc and data/genes.json with the reference's variable set, 2 adds the
    qd_* extension variables with which the ecology lanes resume bit for bit (qingdai_amd/ecology.py persist_level).  Under
    QD_CHECKPOINT=1 the level is 2 whatever the variable says: ecology.nc and genes.json then fit the checkpoint beside them."""
    from .ecology import persist_level
    from .checkpoint import read_env
    return 2 if read_env(env)["enabled"] else persist_level(env)


def indiv_daily_enabled(env, *, eco_daily, ecology, population, individuals, daily_hook):
    """QD_ECO_INDIV_DAILY (default 0): 1 runs IndividualPool.step_daily on the device behind every firing of the daily vegetation
    lane.  It acts on that lane's resident stack, so it is refused without what the lane and the pool need."""
    if int(env.get("QD_ECO_INDIV_DAILY", "0")) != 1:
        return False
    missing = [what for ok, what in ((ecology, "QD_ECO_ENABLE=1"), (population, "a population (QD_ECO_USE_LAI=1)"),
                                     (individuals, "individuals (QD_ECO_INDIV_ENABLE=1)"), (not daily_hook, "no daily_hook"),
                                     (eco_daily, "QD_ECO_DAILY=1")) if not ok]
    if missing:
        raise ValueError("QD_ECO_INDIV_DAILY=1 needs " + ", ".join(missing) + ": the individuals' daily step runs behind the device "
                         "daily vegetation step on its resident stack; set what is missing or unset QD_ECO_INDIV_DAILY")
    return True


def topo_device(env):
    """QD_TOPO_DEVICE (default 0): 1 builds the procedural planet on the device (qingdai_amd/topogen.py)."""
    return int(env.get("QD_TOPO_DEVICE", "0")) == 1


def hydro_autogen(env):
    """QD_HYDRO_AUTOGEN (default 0): 1 generates a missing network file, as the reference driver always does."""
    return int(env.get("QD_HYDRO_AUTOGEN", "0")) == 1


def plots_line(stateframe, truecolor, sim, figures=None):
    """The [Plots] start-up line.  Without the figures it is one of the three wordings it always had."""
    if figures is not None:
        names, _ = sim.figure_names()
        what = [w for w, on in (("the 15-panel state frame (state_day_*.png + .json, no axes)", stateframe is not None),
                                ("the true-colour frame", truecolor is not None)) if on]
        what.append(("the " + ", ".join(names) + " figures (tiles + .json, no axes)") if names else "no further figure (every QD_FIGURES switch is off)")
        return (f"[Plots] {'; '.join(what)}: produced by the device driver, every {sim.plot_every} steps; the reference's plot_ocean "
                "is never called and is not.")
    if stateframe is None:
        if truecolor is None:
            return "[Plots] matplotlib panels are not produced by the device driver (out of the hot path)."
        return (f"[Plots] only the true-colour frame is produced by the device driver, every {sim.plot_every} steps; "
                "the matplotlib panels are not.")
    what = "the 15-panel state frame (state_day_*.png + .json, no axes)" + (" and the true-colour frame" if truecolor is not None else "")
    return (f"[Plots] {what} produced by the device driver, every {sim.plot_every} steps; the ocean, plankton, ISR and ecology "
            "figures are not.")


def chunk_until(t, dt, next_autosave_t, remaining, max_chunk=200, fire_in=None):
    """Steps to hand to the device loop in one go: at most `max_chunk`, at most `remaining`, and -- when a periodic autosave is
    pending -- exactly up to the step whose END reaches the threshold (the reference tests `t >= next_autosave_t` at the top of the
    following step, run_simulation.py:1762), at least one.  fire_in (Simulation.diversity_due): the chunk ends no later than the
    step that fires the diversity diagnostics, which run on the state after that step."""
    n = min(max_chunk, remaining)
    if next_autosave_t is not None:
        to_thr = int(np.ceil((next_autosave_t - t) / dt - 1e-9))
        if to_thr > 0:
            n = max(1, min(n, to_thr))
    if fire_in is not None and fire_in >= 1:
        n = min(n, int(fire_in))
    return n


def main(argv=None):
    env = os.environ
    print("--- Initializing Qingdai GCM (MI355X device path) ---")
    # P020 Phase-0 switch (run_simulation.py:1172-1191): the facade only advances a clock
    if int(env.get("QD_USE_OO", "0")) == 1 and int(env.get("QD_USE_OO_STRICT", "0")) == 1:
        print("[P020] QD_USE_OO=1 QD_USE_OO_STRICT=1 -> facade stub only; exiting legacy engine.")
        return 0
    sim = Simulation()
    day = 2 * np.pi / PLANET_OMEGA
    if env.get("QD_TOTAL_YEARS"):
        duration = float(env["QD_TOTAL_YEARS"]) * sim.forcing.orbital_system.T_planet
    elif env.get("QD_SIM_DAYS"):
        duration = float(env["QD_SIM_DAYS"]) * day
    else:
        duration = 5 * sim.forcing.orbital_system.T_planet
    # run_simulation.py:1451-1563: QD_RESTART_IN wins; else the autosave checkpoint data/atmosphere.nc when QD_AUTOSAVE_LOAD=1 (the
    # default); in both cases data/ocean.nc then overrides the ocean fields when QD_LOAD_OCEAN=1 (default).  Load failures fall back
    # to a fresh start, as in the reference.
    data_dir = env.get("QD_DATA_DIR", "data")
    restart_in = env.get("QD_RESTART_IN")
    autosave_nc = os.path.join(data_dir, "atmosphere.nc")
    # QD_CHECKPOINT=1 (qingdai_amd/checkpoint.py): with QD_AUTOSAVE_LOAD=1 and no QD_RESTART_IN an existing checkpoint file wins over
    # atmosphere.nc, ocean.nc, ecology.nc and plankton.nc -- the run then continues the saved one bit for bit.  A file that does not
    # fit is refused with one line and start-up fails, unless QD_CHECKPOINT_STRICT=0 takes the load order above instead
    from . import checkpoint
    ck = checkpoint.read_env(env, data_dir)
    ck_file = None
    if ck["enabled"]:
        why = checkpoint.startup_refusal(sim, env)
        if why:
            print(f"[Checkpoint] {why}")
            return 2
        if sim.eco is not None and sim.eco.pop is not None:
            from .ecology import persist_level
            if persist_level(env) < 2:
                print("[Checkpoint] ecology.nc and genes.json are written and read as under QD_ECO_PERSIST=2.")
        if not restart_in and int(env.get("QD_AUTOSAVE_LOAD", "1")) == 1 and os.path.exists(ck["path"]):
            try:
                ck_file = checkpoint.read(ck["path"])
                checkpoint.check_grid_and_abi(ck_file, sim.dev.shape, sim.dev)
                checkpoint.verify_file(ck_file)
            except checkpoint.CheckpointRefused as e:
                print(f"[Checkpoint] refused '{ck['path']}': {e}")
                if ck["strict"]:
                    return 2
                ck_file = None

    def _legacy_load():
        loaded = None
        if restart_in and os.path.exists(restart_in):
            loaded = restart_in
        elif not restart_in and int(env.get("QD_AUTOSAVE_LOAD", "1")) == 1 and os.path.exists(autosave_nc):
            loaded = autosave_nc
        if loaded:
            try:
                sim.load(loaded)
                print(f"[{'Restart' if loaded == restart_in else 'Autosave'}] loaded '{loaded}' at t={sim.t:.1f} s")
                if int(env.get("QD_LOAD_OCEAN", "1")) == 1:
                    try:
                        if sim.load_ocean_override(os.path.join(data_dir, "ocean.nc")):
                            print("[Restart] Ocean state overridden from 'data/ocean.nc'.")
                    except Exception as e:     # noqa: BLE001
                        print(f"[Restart] ocean.nc load skipped: {e}")
            except Exception as e:             # noqa: BLE001
                print(f"[Restart] Failed to load '{loaded}': {e}\nContinuing with fresh init.")
                loaded = None
        # run_simulation.py:1464-1488 / 1566-1590: genes.json, then the ecology autosave, behind either checkpoint or none
        # (QD_ECO_PERSIST >= 1; gated by QD_AUTOSAVE_LOAD alone, like the reference)
        sim.load_ecology(data_dir, env)
        # run_simulation.py:1377-1399: data/plankton.nc restores the tracer distributions at startup (QD_LOAD_PLANKTON=1, default)
        if sim.phyto is not None and int(env.get("QD_LOAD_PLANKTON", "1")) == 1:
            pnc = os.path.join(data_dir, "plankton.nc")
            if os.path.exists(pnc):
                loader = sim.phyto_daily if sim.phyto_daily is not None else sim.phyto
                print(f"[Phyto] plankton.nc load {'OK' if loader.load_distribution_nc(pnc) else 'skipped/failed'}.")
        if not loaded and sim.t == 0.0:
            if env.get("QD_ORBIT_EPOCH_SECONDS"):
                sim.t = float(env["QD_ORBIT_EPOCH_SECONDS"])
            elif env.get("QD_ORBIT_EPOCH_DAYS"):
                sim.t = float(env["QD_ORBIT_EPOCH_DAYS"]) * day
    if ck_file is None:
        _legacy_load()
    sim.enable_routing(env)
    sim.enable_budget_diag(env)
    for name in WINDOW_LANES:
        enable = getattr(sim, "enable_" + name, None)          # (a stand-in Simulation from before a lane has none)
        if enable is not None:
            enable(env)
    if ck_file is not None:                                    # behind the lanes: their buffers and clocks come from the file
        try:
            sim.load_checkpoint(ck_file, env)
        except checkpoint.CheckpointRefused as e:
            print(f"[Checkpoint] refused '{ck['path']}': {e}")
            if ck["strict"]:
                return 2
            ck_file = None
            _legacy_load()
    if ck_file is None:                                        # (a resumed run had its bootstrap before its first step)
        sim.bootstrap_ecology()
    t0 = sim.t
    n_total = len(np.arange(t0, t0 + duration, sim.dt))
    print(f"Grid resolution: {sim.grid.n_lat} lat x {sim.grid.n_lon} lon | dt = {sim.dt} s | "
          f"{duration / day:.1f} planetary days | {n_total} steps")
    plots = plots_line(sim.enable_stateframe(env), sim.enable_truecolor(env), sim, sim.enable_figures(env))
    print(plots)

    autosave_on = int(env.get("QD_AUTOSAVE_ENABLE", "1")) == 1
    restart_out = env.get("QD_RESTART_OUT") or os.path.join("data", "restart_autosave.nc")
    # periodic autosave (run_simulation.py:1751-1764): every QD_ECO_AUTOSAVE_EVERY_HOURS PLANETARY hours (day / 24; default 6),
    # tracked as a time threshold -- the first step whose time has reached it saves, whatever the chunking of the device loop
    try:
        every_h = float(env.get("QD_ECO_AUTOSAVE_EVERY_HOURS", "6"))
        autosave_dt = every_h * (day / 24.0) if every_h > 0 else None
    except ValueError:
        autosave_dt = None
    next_autosave_t = t0 + autosave_dt if autosave_dt else None
    state = {"saved": False}

    def _autosave(reason):
        if state["saved"] or not autosave_on:
            return
        try:
            # run_simulation.py:1669-1687: data/atmosphere.nc (+ data/ocean.nc, data/topography.nc); QD_RESTART_OUT on top
            sim.save_autosave(data_dir)
            if env.get("QD_RESTART_OUT"):
                sim.save(restart_out)
            print(f"[Autosave] ({reason}) core state saved to 'data/atmosphere.nc' at t={sim.t:.1f} s")
        except Exception as e:     # noqa: BLE001  (the reference never lets I/O kill the run)
            print(f"[Autosave] skipped: {e}")
        if ck["enabled"]:                                      # behind the reference's files, which are written exactly as before
            try:
                sim.save_checkpoint(ck["path"], reason=reason)
            except Exception as e:     # noqa: BLE001  (not at a span boundary, or I/O: the last good file stays)
                print(f"[Checkpoint] ({reason}) skipped: {e}")
        state["saved"] = True

    def _stop(signum):
        _autosave("signal")
        sys.exit(130 if signum == signal.SIGINT else 143)

    def _on_signal(signum, _frame):
        # Python runs a handler right behind the device call it interrupted, before the span's bookkeeping: the device is then up to
        # a chunk ahead of the host clocks.  The f4 files promise no continuation and are written at once, as always; a run that
        # writes checkpoints waits for the end of the chunk in flight, where both stand at the same step
        if ck["enabled"] and getattr(sim, "request_stop", None) is not None and sim.request_stop(lambda: _stop(signum)):
            return
        _stop(signum)
    signal.signal(signal.SIGINT, _on_signal)
    signal.signal(signal.SIGTERM, _on_signal)
    atexit.register(lambda: _autosave("atexit"))

    wall0 = time.perf_counter()

    def _after_chunk(done, next_autosave_t):
        if int(env.get("QD_DYN_DIAG_PRINT", "1")) == 1:
            dg = sim.diagnostics()
            el = time.perf_counter() - wall0
            print(f"t={sim.t / day:8.2f} d | " + " ".join(f"{k}={v:.4g}" for k, v in dg.items()) +
                  f" | {done / max(el, 1e-9):.0f} steps/s")
        if next_autosave_t is not None and sim.t >= next_autosave_t - 1e-9 * sim.dt and done < n_total:
            state["saved"] = False
            _autosave("periodic")
            state["saved"] = False
            while next_autosave_t <= sim.t + 1e-9 * sim.dt:
                next_autosave_t += autosave_dt
        return next_autosave_t
    sim.run_loop(n_total, next_autosave_t if autosave_on else None, _after_chunk)
    if not (ck["enabled"] and autosave_on):
        # the open windows, marked incomplete (the signal path does not get here); under QD_CHECKPOINT=1 the final checkpoint carries
        # them instead, and the run that resumes writes each when it is complete
        for name in WINDOW_LANES:
            if getattr(sim, name, None) is not None:
                getattr(sim, "flush_" + name)(complete=0)
    if env.get("QD_RESTART_OUT"):
        sim.save(env["QD_RESTART_OUT"])
        print(f"[Restart] wrote {env['QD_RESTART_OUT']}")
    # the reference leaves the final checkpoint to its atexit handler (run_simulation.py:1669-1706); doing it here gives the
    # same files to a caller that invokes main() in-process (the handler then finds the state saved)
    state["saved"] = False
    _autosave("final")
    print("--- Simulation Finished ---")
    return 0


if __name__ == "__main__":
    sys.exit(main())
