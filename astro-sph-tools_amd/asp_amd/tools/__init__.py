"""Mirror of astro_sph_tools.tools: the projection path, the periodic-box helpers it uses
and the cross-snapshot ID matching of _ArrayReorder (tools/__init__.py:5)."""
from . import projections  # noqa: F401
from ._periodic_box_manipulations import (calculate_wrapped_displacement,  # noqa: F401
                                          calculate_wrapped_distance, make_periodic,
                                          calculate_periodic, shift_origin, shift_centre)
from ._ArrayReorder import ArrayReorder, ArrayMapping, match_ids, take_rows  # noqa: F401
