"""MI355X-native LEGACY Monte Carlo engine (citizens'-assembly replication hot path).

The package directory name contains a hyphen, so import it with
``importlib.import_module("citizensassemblies-replication_amd")`` (or add the
directory to ``sys.path``).  Public surface, mirroring the
reference's legacy.py / analysis.py LEGACY functions:

    read_instance, Instance, PairHistogram, SelectionError, check_min_cats,
    find_random_sample_legacy, legacy_find, legacy_probabilities, seed

plus set_rng_mode("mt" | "philox") (the reference's own MT19937 stream on the host, or the
device's Philox verification-mode stream, the default)

plus the analysis side of LEXIMIN / XMIN after the solver (analysis.py:194-228):
leximin_probabilities, xmin_probabilities (solver passed in or imported from the reference)
and portfolio_probabilities, bit-equal float64 sums in portfolio order on the device

plus what a run's panels look like as a whole: legacy_composition(instance, iterations, seed, groups)
returns legacy_probabilities' results and a CompositionHistogram (per agent group -- feature_groups,
intersection_groups, agent_groups -- how many panels hold 0, 1, ..., k of its members), counted on the
device by group_hist_kernel; intersectional_representation gives the numbers of
plot_intersectional_representation (analysis.py:459-530); and the same question for a LEXIMIN / XMIN
portfolio: leximin_composition, xmin_composition, portfolio_composition return the probabilities'
results and a WeightedCompositionHistogram (per group, the summed probability of the panels holding 0,
1, ..., k members, added in portfolio order on the device by whist_count_kernel + whist_sum_kernel, bit
for bit what group_whist_host adds on the host); composition_difference sets two compositions against
each other (LEGACY against LEXIMIN)

plus the run as a distribution over whole panels: legacy_panel_distribution(instance, iterations, seed)
returns legacy_probabilities' results and a PanelDistribution (how often each distinct panel was drawn,
from uq_mult_kernel / unique_mult_kernel and mult_spectrum_kernel on the device: the multiplicity
spectrum, sample coverage, the Chao1 bound on the panels possible, the most frequent panels);
panel_multiplicities_host is the same list in numpy

plus two such tables side by side (csa_rows_join_async / csa_rows_find_async over the sorted distinct
rows): PanelSet's set operators and comparisons, legacy_panel_comparison(instance, iterations) -- two
seeds and their PanelComparison (shared panels, held-out coverage, overlap, cross-sample collision) --
and legacy_portfolio_overlap, a run beside a LEXIMIN / XMIN portfolio (PortfolioOverlap)

plus a weight per agent against such a table (csa_rows_price_async / csa_rows_mw_cover_async /
csa_rows_first_holder_async): PanelDistribution.price(weights) -- the drawn panel with the largest weight
sum, the heuristic pricing step of LEXIMIN / XMIN's column generation --, initial_committees(rounds), the
reference's multiplicative-weights stage over the drawn panels (legacy_initial_committees), and
legacy_price over fresh draws that are not kept; rows_*_host are the numpy contracts

plus the maximin lottery over such a table (csa_rows_maximin_async): PanelDistribution.maximin(rounds) /
legacy_maximin -- how fair a lottery over exactly the drawn panels can be made, the reference's first leximin
stage over them solved by multiplicative weights with a lower and an upper bound (PanelMaximin), no LP
solver; rows_maximin_host is the numpy contract

plus the Nash-welfare lottery over such a table (csa_rows_nash_async, csa_rows_marginals_async):
PanelDistribution.nash(rounds) / legacy_nash -- the lottery over exactly the drawn panels with the greatest
geometric mean of selection probabilities, by Cover's multiplicative iteration with a certificate
geometric_mean <= optimum <= upper (PanelNash, NashState), no solver; rows_nash_host and rows_marginals_host
are the numpy contracts

plus xmin._get_panel_not_in_portfolio_if_possible (XMIN's LEGACY caller,
xmin.py:464-474) on the device.
"""
from .instance import Instance, read_instance, encode  # noqa: F401
from .legacy import SelectionError, check_min_cats, find_random_sample_legacy, seed, set_rng_mode  # noqa: F401
from .analysis import PairHistogram, PanelSet, legacy_find, legacy_find_batch, legacy_probabilities  # noqa: F401
from .analysis import leximin_probabilities, portfolio_probabilities, xmin_probabilities  # noqa: F401
from .analysis import legacy_composition, legacy_panel_distribution  # noqa: F401
from .analysis import leximin_composition, portfolio_composition, xmin_composition  # noqa: F401
from .stats import (CompositionHistogram, GroupSet, agent_groups, feature_groups, group_composition,  # noqa: F401
                    intersection_groups, intersectional_representation)
from .stats import (WeightedCompositionHistogram, composition_difference, group_whist_host,  # noqa: F401
                    portfolio_group_composition)
from .stats import PanelDistribution, panel_multiplicities_host  # noqa: F401
from .analysis import legacy_panel_comparison, legacy_portfolio_overlap  # noqa: F401
from .stats import (PanelComparison, PortfolioOverlap, compare_panel_distributions, portfolio_overlap,  # noqa: F401
                    rows_find_host, rows_join_host)
from .analysis import legacy_initial_committees, legacy_price  # noqa: F401
from .stats import (PanelPrice, rows_first_holder_host, rows_mw_cover_host, rows_price_host,  # noqa: F401
                    rows_score_host)
from .analysis import legacy_maximin  # noqa: F401
from .stats import MaximinState, PanelMaximin, rows_maximin_host  # noqa: F401
from .analysis import legacy_nash  # noqa: F401
from .stats import NashState, PanelNash, rows_marginals_host, rows_nash_host  # noqa: F401
from .stats import household_groups  # noqa: F401
from . import _native, xmin  # noqa: F401

__all__ = ["Instance", "read_instance", "encode", "SelectionError", "check_min_cats",
           "find_random_sample_legacy", "seed", "set_rng_mode", "PairHistogram", "PanelSet", "legacy_find",
           "legacy_find_batch", "legacy_probabilities", "leximin_probabilities", "xmin_probabilities",
           "portfolio_probabilities", "legacy_composition", "CompositionHistogram", "GroupSet", "agent_groups",
           "feature_groups", "group_composition", "intersection_groups", "intersectional_representation",
           "leximin_composition", "xmin_composition", "portfolio_composition", "WeightedCompositionHistogram",
           "composition_difference", "group_whist_host", "portfolio_group_composition",
           "legacy_panel_distribution", "PanelDistribution", "panel_multiplicities_host",
           "legacy_panel_comparison", "legacy_portfolio_overlap", "PanelComparison", "PortfolioOverlap",
           "compare_panel_distributions", "portfolio_overlap", "rows_join_host", "rows_find_host",
           "legacy_initial_committees", "legacy_price", "PanelPrice", "rows_score_host", "rows_price_host",
           "rows_mw_cover_host", "rows_first_holder_host", "legacy_maximin", "PanelMaximin", "MaximinState",
           "rows_maximin_host", "household_groups", "legacy_nash", "PanelNash", "NashState", "rows_nash_host",
           "rows_marginals_host"]
