"""Diagnostics post-processors (mirror of xanthos/diagnostics): runoff totals against four comparison data sets, and the
time-series plots of the written runoff and channel flow."""
