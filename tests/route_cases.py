"""The launches whose kernel choice tests/test_routes.py pins: one dict per case, read by the host probe (tests/route_probe.hip, through
`probe_line`) and by whoever replays the list on a GPU to record the kernels a build launches.

A case: id, entry ('filter' | 'filter_split' | 'smoother' | 'smoother_split' | 'select'), method and model by name, the sigma-point set by
kind, B, T, flags, requested segments, the byte offset of the record pointers from a 16-byte boundary, num_cus, for 'select' whether
mss / Pss are NULL, and for the smoothers' plan what the occupancy query of the walks' launcher would say (blocks_per_cu, 0: it failed), the
context's CGP_DBG_WALK_SEGMENTS value (walk_cap) and the burn-in of a 'smoother_split'.  `run`: a 256-CU GPU can replay the case cheaply (the others -- another CU count, records of gigabytes, a constructed
sigma-point set -- have their expected route derived by reading the dispatch code, "derived" in tests/golden/routes.json)."""

WAVE, THREAD, SEQUENTIAL_SCAN, GENERIC, LITERAL_SIGMA_SUM, DPP = 0x2, 0x4, 0x8, 0x10, 0x40, 0x80
FOUR_TRIALS, ONE_TRIAL, TIME_SPLIT, NO_TIME_SPLIT = 0x200, 0x400, 0x800, 0x1000
FLAG_SETS = {'none': 0, 'wave': WAVE, 'thread': THREAD, 'generic': GENERIC, 'dpp': DPP, 'four': FOUR_TRIALS, 'one': ONE_TRIAL,
             'seq': SEQUENTIAL_SCAN, 'split': TIME_SPLIT, 'nosplit': NO_TIME_SPLIT, 'literal': LITERAL_SIGMA_SUM}

FILTERS = {'ekf': 0, 'sgp': 1, 'cd_ekf': 2, 'cd_sgp': 3, 'ekf_kpt': 4}
SMOOTHERS = {'eks': 0, 'sgp': 1, 'cd_eks': 2, 'cd_sgp': 3}
SIGMA_STANDARD, SIGMA_AXIAL = 0x1, 0x2
KOOB = 0x7FFFFF00                      # the 2 GiB raw-buffer window of include-side kernels, quoted (csrc: kOobMaxBytes)

# model name -> (model_id, d, n_harm, kind); kind: 'disc' (ekf / sgp), 'sde' (cd_*), 'kpt'
MODELS = {
    'linear3': (0, 3, 0, 'disc'), 'linear4': (0, 4, 0, 'disc'), 'linear6': (0, 6, 0, 'disc'),
    'chirp': (1, 4, 1, 'disc'), 'lascala': (2, 4, 1, 'disc'), 'harm2': (1, 6, 2, 'disc'), 'harm3': (1, 8, 3, 'disc'), 'harm4': (1, 10, 4, 'disc'),
    'linear_sde4': (3, 4, 0, 'sde'), 'chirp_sde1': (4, 4, 1, 'sde'), 'chirp_sde2': (4, 6, 2, 'sde'),
    'kpt1': (5, 3, 1, 'kpt'), 'kpt2': (5, 4, 2, 'kpt'), 'kpt3': (5, 5, 3, 'kpt'),
}
NONLINEAR = {1, 2, 4}                  # model ids whose sets the Python layer groups by the coordinates in front of the last one


def sigma_shape(kind, model):
    """(s, n_groups, grouped, flags) of the cgp_sigma a case hands over; None: no set."""
    model_id, d = MODELS[model][0], MODELS[model][1]
    grouped = model_id in NONLINEAR
    if kind is None:
        return None
    if kind == 'gh3':                  # Gauss-Hermite, order 3: 3^d points, groups of three
        return (3 ** d, 3 ** (d - 1), True, SIGMA_STANDARD) if grouped else (3 ** d, 0, False, 0)
    if kind == 'cub':                  # cubature: 2 d points on the axes; +- e_d share a group
        return (2 * d, 2 * d - 1, True, SIGMA_STANDARD | SIGMA_AXIAL) if grouped else (2 * d, 0, False, 0)
    if kind == 'ungrouped':            # GH-3 handed over without groups (and so without the standard-set assertion)
        return (3 ** d, 0, False, 0)
    if kind == 'g33':                  # a standard set with one group more than the matrix-core kernels' 32
        return (99, 33, True, SIGMA_STANDARD)
    if kind == 'big':                  # Gauss-Hermite, order 6: beyond the 44 KiB LDS stage of the wave-per-trial kernels at d = 4
        return (6 ** d, 6 ** (d - 1), True, SIGMA_STANDARD) if grouped else (6 ** d, 0, False, 0)
    raise ValueError(kind)


CASES = []


def case(id, entry, method, model, sigma=None, B=4, T=128, flags=0, segments=1, align=0, num_cus=256, null_rows=False, run=True,
         blocks_per_cu=4, walk_cap=0, burn_in=0):
    assert id not in {c['id'] for c in CASES}, id
    CASES.append(dict(id=id, entry=entry, method=method, model=model, sigma=sigma, B=B, T=T, flags=flags, segments=segments, align=align,
                      num_cus=num_cus, null_rows=null_rows, run=run and num_cus == 256 and sigma != 'g33',
                      blocks_per_cu=blocks_per_cu, walk_cap=walk_cap, burn_in=burn_in))


def methods_of(model):
    kind = MODELS[model][3]
    return {'disc': (('ekf', 'sgp'), ('eks', 'sgp')), 'sde': (('cd_ekf', 'cd_sgp'), ('cd_eks', 'cd_sgp')), 'kpt': (('ekf_kpt',), ())}[kind]


def default_sigma(method, model):
    if 'sgp' not in method:
        return None
    return 'gh3' if MODELS[model][1] <= 4 else 'cub'


# ---- methods x models x flags
for _model in MODELS:
    _filters, _smoothers = methods_of(_model)
    for _fname, _flags in FLAG_SETS.items():
        for _m in _filters:
            case(f'f-{_m}-{_model}-{_fname}', 'filter', _m, _model, default_sigma(_m, _model), flags=_flags)
        for _m in _smoothers:
            case(f's-{_m}-{_model}-{_fname}', 'smoother', _m, _model, default_sigma(_m, _model), flags=_flags)

# ---- sigma-point sets
for _model, _f, _s in (('chirp', 'sgp', 'sgp'), ('harm2', 'sgp', 'sgp'), ('chirp_sde1', 'cd_sgp', 'cd_sgp')):
    for _kind in ('gh3', 'ungrouped', 'g33', 'big'):
        if _kind == 'big' and _model == 'harm2':
            continue                                   # 46 656 points: the d = 4 models cover the LDS-stage bound
        for _fname in ('none', 'thread', 'dpp', 'literal'):
            case(f'f-{_f}-{_model}-{_kind}-{_fname}', 'filter', _f, _model, _kind, flags=FLAG_SETS[_fname])
            case(f's-{_s}-{_model}-{_kind}-{_fname}', 'smoother', _s, _model, _kind, flags=FLAG_SETS[_fname])

# ---- record shapes: the lane kernels take even T and 16-byte aligned records only
for _T in (128, 130, 127):
    for _align in (0, 8):
        for _m, _model in (('ekf', 'chirp'), ('sgp', 'chirp'), ('ekf', 'lascala')):
            case(f'f-{_m}-{_model}-lane-T{_T}-a{_align}', 'filter', _m, _model, default_sigma(_m, _model), B=70, T=_T, flags=THREAD, align=_align)
        for _m, _model in (('eks', 'chirp'), ('cd_eks', 'chirp_sde1'), ('sgp', 'chirp')):
            case(f's-{_m}-{_model}-lane-T{_T}-a{_align}', 'smoother', _m, _model, default_sigma(_m, _model), B=70, T=_T, flags=THREAD, align=_align)

# ---- selected outputs with mss / Pss NULL: native in the walks, the tile-layout and the lane kernels, refused elsewhere
for _m, _model in (('eks', 'chirp'), ('sgp', 'chirp'), ('eks', 'linear4'), ('eks', 'linear6'), ('eks', 'harm2'), ('eks', 'linear3'),
                   ('cd_eks', 'chirp_sde1'), ('cd_sgp', 'chirp_sde1'), ('eks', 'harm4')):
    for _fname in ('none', 'thread', 'generic'):
        case(f'sel-{_m}-{_model}-{_fname}', 'select', _m, _model, default_sigma(_m, _model), flags=FLAG_SETS[_fname], null_rows=True)

# ---- time split with burn-in, two segments: the four admitted filters, two refused ones; the smoothers' two and one refused
for _m, _model, _flags in (('ekf', 'chirp', 0), ('sgp', 'chirp', 0), ('sgp', 'harm2', 0), ('cd_sgp', 'chirp_sde1', 0), ('ekf', 'lascala', 0),
                           ('cd_ekf', 'chirp_sde1', 0), ('ekf', 'chirp', DPP), ('sgp', 'harm2', DPP), ('ekf', 'chirp', FOUR_TRIALS),
                           ('ekf', 'harm2', 0), ('ekf', 'chirp', ONE_TRIAL)):
    case(f'fsplit-{_m}-{_model}-{_flags:x}', 'filter_split', _m, _model, default_sigma(_m, _model), T=256, flags=_flags, segments=2)
case('fsplit-ekf-chirp-short', 'filter_split', 'ekf', 'chirp', T=64, segments=2)              # one effective segment
case('fsplit-ekf-chirp-short-b2048', 'filter_split', 'ekf', 'chirp', B=2048, T=64, segments=2)
for _m, _model, _flags in (('cd_eks', 'chirp_sde1', 0), ('cd_sgp', 'chirp_sde1', 0), ('cd_eks', 'chirp_sde1', DPP), ('cd_sgp', 'chirp_sde1', DPP),
                           ('eks', 'chirp', 0), ('cd_eks', 'chirp_sde2', 0)):
    case(f'ssplit-{_m}-{_model}-{_flags:x}', 'smoother_split', _m, _model, default_sigma(_m, _model), T=256, flags=_flags, segments=2)

# ---- crossovers between one wavefront and one lane per trial: the first B that runs one lane per trial is num x (4 num_cus) / den
#      trials (cgp_api.hip at the parent of this test: lines 11-25, 404-415, 536-544).  T = 64; an odd T or misaligned rows keep the
#      d = 4 lane kernels out, which moves the d = 4 limits from 9 / 9 / 3 to 20 / 24 / 5.
CROSSOVERS = (
    # id, entry, method, model, T, align, num, den
    ('ekf4-lane4', 'filter', 'ekf', 'chirp', 64, 0, 9, 1), ('ekf4', 'filter', 'ekf', 'chirp', 63, 0, 20, 1),
    ('sgp4-lane4', 'filter', 'sgp', 'chirp', 64, 0, 9, 1), ('sgp4', 'filter', 'sgp', 'chirp', 63, 0, 24, 1),
    ('ekf8', 'filter', 'ekf', 'harm2', 64, 0, 8, 1), ('sgp8', 'filter', 'sgp', 'harm2', 64, 0, 11, 1),
    ('cdekf4', 'filter', 'cd_ekf', 'chirp_sde1', 64, 0, 4, 1), ('cdsgp4', 'filter', 'cd_sgp', 'chirp_sde1', 64, 0, 48, 1),
    ('cdeks4-lane4', 'smoother', 'cd_eks', 'chirp_sde1', 64, 0, 3, 1), ('cdeks4', 'smoother', 'cd_eks', 'chirp_sde1', 64, 8, 5, 1),
    ('eks4-lane4', 'smoother', 'eks', 'chirp', 64, 0, 24, 1), ('cdsgps4', 'smoother', 'cd_sgp', 'chirp_sde1', 64, 0, 48, 1),
    ('generic-ekf', 'filter', 'ekf', 'linear3', 64, 0, 5, 2), ('generic-sgp', 'filter', 'sgp', 'linear3', 64, 0, 8, 1),
    ('generic-kpt', 'filter', 'ekf_kpt', 'kpt3', 64, 0, 5, 2), ('generic-cdeks', 'smoother', 'cd_eks', 'linear_sde4', 64, 0, 5, 2),
    ('generic-cdsgps', 'smoother', 'cd_sgp', 'linear_sde4', 64, 0, 8, 1), ('generic-scan', 'smoother', 'eks', 'linear3', 64, 0, 16, 1),
)
for _id, _entry, _m, _model, _T, _align, _num, _den in CROSSOVERS:
    for _cus in (256, 8):
        _first_lane = -(-_num * 4 * _cus // _den)
        for _B in (_first_lane - 1, _first_lane):
            case(f'x-{_id}-cu{_cus}-B{_B}', _entry, _m, _model, default_sigma(_m, _model), B=_B, T=_T, align=_align, num_cus=_cus)
# the four-trials-per-wavefront EKF: above 1024 trials whatever the CU count
for _cus in (256, 8):
    for _B in (1024, 1025):
        case(f'x-ekf4-x4-cu{_cus}-B{_B}', 'filter', 'ekf', 'chirp', B=_B, T=64, flags=WAVE, num_cus=_cus)
# the discrete smoothers on the cooperative walks never cross over
for _m, _model in (('eks', 'linear4'), ('eks', 'linear6'), ('sgp', 'harm2'), ('sgp', 'chirp')):
    case(f'x-walk-{_m}-{_model}', 'smoother', _m, _model, default_sigma(_m, _model), B=40000, T=64)

# ---- window edges: the longest record a kernel's 2 GiB output window takes, one step less and one more (never run: gigabytes)
EDGES = (
    # id, entry, method, model, B, flags, bytes per step that the window has to hold
    ('ekf4', 'filter', 'ekf', 'chirp', 4, 0, 128), ('kf4', 'filter', 'ekf', 'linear4', 4, 0, 128), ('sgp4', 'filter', 'sgp', 'chirp', 4, 0, 128),
    ('cdekf4', 'filter', 'cd_ekf', 'chirp_sde1', 4, 0, 128), ('cdsgp4', 'filter', 'cd_sgp', 'chirp_sde1', 4, 0, 128),
    ('cdeks4', 'smoother', 'cd_eks', 'chirp_sde1', 4, 0, 128), ('cdsgps4', 'smoother', 'cd_sgp', 'chirp_sde1', 4, 0, 128),
    ('walk4', 'smoother', 'eks', 'chirp', 4, 0, 128), ('walk4-linear', 'smoother', 'eks', 'linear4', 4, 0, 128),
    ('ekf4-x4', 'filter', 'ekf', 'chirp', 2048, 0, 512),
    ('ekf8-d6', 'filter', 'ekf', 'harm2', 4, 0, 6 * 6 * 8), ('ekf8-d8', 'filter', 'ekf', 'harm3', 4, 0, 8 * 8 * 8), ('sgp8-d6', 'filter', 'sgp', 'harm2', 4, 0, 6 * 6 * 8),
    ('kpt1', 'filter', 'ekf_kpt', 'kpt1', 4, 0, 3 * 3 * 8), ('kpt2', 'filter', 'ekf_kpt', 'kpt2', 4, 0, 4 * 4 * 8), ('kpt3', 'filter', 'ekf_kpt', 'kpt3', 4, 0, 5 * 5 * 8),
    ('coop8-linear6', 'smoother', 'eks', 'linear6', 4, 0, 6 * 6 * 8), ('coop8-harm2', 'smoother', 'eks', 'harm2', 4, 0, 6 * 6 * 8),
    ('lane4-ekf', 'filter', 'ekf', 'chirp', 70, THREAD, 128 * 64), ('lane4-eks', 'smoother', 'eks', 'chirp', 70, THREAD, 128 * 64),
    ('lane4-limit', 'filter', 'ekf', 'chirp', 9216, 0, 128 * 64),
)
for _id, _entry, _m, _model, _B, _flags, _row in EDGES:
    for _dT in (-1, 0, 1):
        case(f'edge-{_id}-{_dT:+d}', _entry, _m, _model, default_sigma(_m, _model), B=_B, T=KOOB // _row + _dT, flags=_flags, run=False)

# ---- the smoothers' launch plan, one case each way across every edge of it (never run: their answers are worked out by hand from the code
#      that decided them before route_smoother did -- smoother_impl, walk_segments and launch_walk_smoother at the parent of these cases)
# The exact split of the walks (eks on the chirp model unless said; T = 577 is nine 64-step tiles, T = 3201 fifty).
for _cus, _B in ((256, 341), (256, 342), (8, 10), (8, 11)):                # splits while 3 B <= 4 num_cus
    case(f'plan-cutoff-cu{_cus}-B{_B}', 'smoother', 'eks', 'chirp', B=_B, T=577, num_cus=_cus, run=False)
case('plan-linear4-none', 'smoother', 'eks', 'linear4', T=577, run=False)                 # the caller's F: not by default ...
case('plan-linear4-split', 'smoother', 'eks', 'linear4', T=577, flags=TIME_SPLIT, run=False)              # ... but on request
case('plan-split-nosplit', 'smoother', 'eks', 'chirp', T=577, flags=TIME_SPLIT | NO_TIME_SPLIT, run=False)
case('plan-cap1', 'smoother', 'eks', 'chirp', T=577, walk_cap=1, run=False)
case('plan-cap0', 'smoother', 'eks', 'chirp', T=577, run=False)                           # (what plan-cap1 switches off)
case('plan-cap5', 'smoother', 'eks', 'chirp', B=125, T=3201, walk_cap=5, run=False)       # a cap that binds: 8 segments without it
case('plan-quoted', 'smoother', 'eks', 'chirp', B=125, T=3201, run=False)                 # the shape of the cut-off's measurement: 8 x 7 tiles
for _T in (4097, 8193):                                                    # 64 and 128 tiles, one each on request: 64 segments at the most
    case(f'plan-ceiling-T{_T}', 'smoother', 'eks', 'chirp', T=_T, flags=TIME_SPLIT, run=False)
for _per_cu in (0, 2, 8, 9):                                               # the occupancy query: 0 is taken as 4, more than 8 as 8
    case(f'plan-percu{_per_cu}', 'smoother', 'eks', 'chirp', B=250, T=3201, blocks_per_cu=_per_cu, run=False)
for _T in (449, 513):                                                      # 7 and 8 tiles: four tiles a segment unless forced
    case(f'plan-mintiles-T{_T}', 'smoother', 'eks', 'chirp', T=_T, run=False)
case('plan-mintiles-T449-split', 'smoother', 'eks', 'chirp', T=449, flags=TIME_SPLIT, run=False)
case('plan-no-empty', 'smoother', 'eks', 'chirp', T=577, flags=TIME_SPLIT, walk_cap=4, run=False)     # 9 tiles on 4 segments: 3 each, so 3 segments
case('plan-coop8', 'smoother', 'sgp', 'harm2', 'cub', B=125, T=3201, run=False)           # the tile-layout walk takes the same plan
case('plan-lane4', 'smoother', 'eks', 'chirp', B=125, T=3201, flags=THREAD | TIME_SPLIT, run=False)   # no walk, no exact split
# The split with burn-in (cd_eks on the chirp SDE): whole 64-step chunks of the T - 1 backward steps, no empty segment.
for _T, _segments in ((64, 2), (65, 2), (66, 2), (129, 2), (257, 10), (321, 3), (321, 4)):
    case(f'plan-burn-T{_T}-s{_segments}', 'smoother_split', 'cd_eks', 'chirp_sde1', T=_T, segments=_segments, run=False)
for _burn_in in (1, 64, 65, -1):
    case(f'plan-burn-in{_burn_in}', 'smoother_split', 'cd_eks', 'chirp_sde1', T=257, segments=2, burn_in=_burn_in, run=False)
case('plan-burn-two-wrongs', 'smoother_split', 'eks', 'chirp', T=257, segments=2, burn_in=-1, run=False)      # the burn-in is checked first
# Selected outputs with full rows: written by the kernels that can, gathered behind the others.
case('plan-sel-rows-walk4', 'select', 'eks', 'chirp', run=False)
case('plan-sel-rows-generic', 'select', 'eks', 'linear3', run=False)


def probe_line(c):
    """One line of the probe's input: entry, method, model_id, d, n_harm, then the sigma set (s, n_groups, grouped, flags; s = 0: none), then
    B, T, flags, segments, align, num_cus, null_rows, blocks_per_cu, walk_cap, burn_in (the last three: 4, 0, 0 where a case has none)."""
    model_id, d, n_harm, _ = MODELS[c['model']]
    s, n_groups, grouped, sflags = sigma_shape(c['sigma'], c['model']) or (0, 0, False, 0)
    method = (SMOOTHERS if c['entry'] in ('smoother', 'smoother_split', 'select') else FILTERS)[c['method']]
    fields = (c['entry'], method, model_id, d, n_harm, s, n_groups, int(grouped), sflags, c['B'], c['T'], c['flags'], c['segments'], c['align'],
              c['num_cus'], int(c['null_rows']), c.get('blocks_per_cu', 4), c.get('walk_cap', 0), c.get('burn_in', 0))
    return ' '.join(str(f) for f in fields)
