"""Scoring a forward run against measurements ([Evaluate]): the routed streamflow at stream gauges."""
from .gauge_skill import (COLUMNS, FLOW_FILE, SKILL_FILE, GaugeSkill, check_routes, load_gauge_set, month_labels,  # noqa: F401
                          skill_fields, skill_table, write_flow, write_skill)
