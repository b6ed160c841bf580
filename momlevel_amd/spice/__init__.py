"""momlevel.spice on the MI355X: seawater spiciness (the reference's src/momlevel/spice)."""

from . import flament

__all__ = ["flament"]
