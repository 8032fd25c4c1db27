"""Hydropower post-processors (mirror of xanthos/hydropower): potential and actual hydropower from the routed channel flow."""
